"""``strandedness`` / ``-s auto`` on the device: ``spl_strand_tally`` on fused sets against the yardstick of ``strandcases.py`` --
exactly, the sums being integers -- at the sizes where the kernel's geometry changes, on reads of every kind with and without
either source of evidence and cover maps below and beyond its LDS top level, in any order of the reads; its refusals; the three
decodes and SAM text through ``tally_of_source``; the commands on synthetic libraries of known strandedness."""
import os

import numpy as np
import pytest

import strandcases as S
import xscases as X
from spliser_amd import cli, native, process as proc, samio, strandedness as sd

pytestmark = pytest.mark.gpu

# The kernel's geometry (csrc/spl_strand.h): a workgroup takes SPL_STRAND_TILE = 256 reads a grid-stride step, a read a lane, and a
# launch has at most SPL_STRAND_GRID_MAX = 1024 workgroups.  So the last workgroup of a set is full at 256, and EVERY workgroup
# takes a second step from 1024 * 256 + 1023 * 256 + 1 = 524 033 reads on; 524 289 = 2 * 1024 * 256 + 1 gives the first one a third.
TILE, GRID_MAX = 256, 1024
LARGE = 2 * GRID_MAX * TILE + 1
TOP = 1024          # SPL_STRAND_TOP: entries of a cover map's top level in LDS; a map beyond it is searched in global memory too


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


def _device_tally(ctx, rs, xs, cover):
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, xs=xs)], with_strand=xs is not None) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            got = dr.strand_tally(cover)
            if rs.n:
                assert dr.layout_bytes()[1] == 0          # (the set stays fused)
            return got.tolist()


def _random_cover(rng, n, span=200000):
    start = np.sort(rng.choice(np.arange(1, span), n, replace=False)).astype(np.int32)
    return start, rng.integers(0, 4, n).astype(np.uint8)


def _case_b():
    """The 4200 reads of test_gpu_aux_strand's case b: spliced reads around the 256th and the 2048th, two reads of 2 203 ops."""
    recs, xs = [], []
    for i in range(4200):
        pos = 1000 + 10 * i
        if i in (255, 256, 257, 2047, 2048, 2049, 300, 2100) or i % 37 == 0:
            recs.append((16 if i % 2 else 0, pos, "%dM%dN%dM" % (10 + i % 9, 200 + (i % 3) * 50, 12 + i % 5)))
            xs.append([43, 45, 0][i % 3] if i not in (255, 257, 2047, 2049) else 43 if i < 1000 else 45)
        elif i in (1000, 2050):
            recs.append((0, pos, "1M1I" * 1100 + "5M300N7M"))
            xs.append(45 if i == 1000 else 0)
        else:
            recs.append((0, pos, "50M"))
            xs.append([0, 43][i % 2])
    return samio.ReadSet.from_records(recs), np.asarray(xs, np.uint8)


def _concat(a, b):
    off = np.concatenate((a.cig_off.astype(np.int64), b.cig_off[1:].astype(np.int64) + int(a.cig_off[-1])))
    return samio.ReadSet(np.concatenate((a.pos, b.pos)), np.concatenate((a.flag, b.flag)), off, np.concatenate((a.cigar, b.cigar)))


def _permuted(rs, xs, perm):
    n_ops = np.diff(rs.cig_off.astype(np.int64))[perm]
    off = np.concatenate(([0], np.cumsum(n_ops)))
    take = np.repeat(rs.cig_off.astype(np.int64)[perm] - off[:-1], n_ops) + np.arange(int(off[-1]))
    return samio.ReadSet(rs.pos[perm], rs.flag[perm], off, rs.cigar[take]), xs[perm]


@pytest.fixture(scope="module")
def content():
    """Reads of every kind (``xscases.make_reads``: flags 0, 16, 99, 147, 83, 163, 256, 4) with a tag byte on spliced and unspliced
    reads alike, then case b's; a cover map of every size; the yardstick's answers, computed once."""
    rng = np.random.default_rng(20261018)
    a = X.make_reads(rng, 3000, long_cigar_every=97)
    b, xs_b = _case_b()
    rs = _concat(a, b)
    xs = np.concatenate((rng.choice(np.array([0, 43, 45], np.uint8), a.n), xs_b))
    assert set(rs.flag.tolist()) == {0, 16, 99, 147, 83, 163, 256, 4} and int(np.diff(rs.cig_off.astype(np.int64)).max()) == 2203
    covers = {1000: _random_cover(rng, 1000)}
    covers[1] = (np.array([500], np.int32), np.array([2], np.uint8))
    covers[2] = (np.array([300, 60000], np.int32), np.array([1, 2], np.uint8))
    covers[3] = (np.array([300, 40000, 90000], np.int32), np.array([1, 3, 2], np.uint8))
    # 40 000 entries of which a read can still lie in a stretch: a thousand clusters of forty entries a base apart, each followed
    # by a stretch of a hundred bases or more -- the top level in LDS finds the cluster, the search in global memory the entry
    anchors = 200 * np.arange(1, 1001) + rng.integers(0, 50, 1000)
    covers[40000] = ((anchors[:, None] + np.arange(40)[None, :]).ravel().astype(np.int32), rng.integers(0, 4, 40000).astype(np.uint8))
    assert (np.diff(covers[40000][0]) > 0).all()
    return rs, xs, covers


# ---- sizes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_sizes_around_a_wave_and_a_tile(ctx, n):
    rng = np.random.default_rng(100 + n)
    rs = X.make_reads(rng, n) if n else samio.ReadSet.empty()
    xs = rng.choice(np.array([0, 43, 45], np.uint8), n)
    cover = _random_cover(rng, 50, 160000)
    want = S.tally(rs, xs, cover)
    assert want[0] == n
    assert _device_tally(ctx, rs, xs, cover) == want
    assert _device_tally(ctx, rs, xs, None) == S.tally(rs, xs, None)


def test_a_set_that_gives_every_workgroup_more_than_one_step(ctx):
    """LARGE reads, built as arrays: six in seven one aligned op, every seventh spliced; the map has 1000 entries."""
    rng = np.random.default_rng(7)
    n = LARGE
    pos = np.sort(rng.integers(1, 3000000, n)).astype(np.int32)
    flag = rng.choice(np.array([0, 16, 99, 147, 83, 163, 256, 4, 1024, 512, 2048], np.uint16), n)
    spliced = np.arange(n) % 7 == 3
    n_ops = np.where(spliced, 3, 1)
    off = np.concatenate(([0], np.cumsum(n_ops)))
    cigar = np.full(int(off[-1]), (50 << 4) | 0, np.uint32)
    cigar[off[:-1][spliced] + 1] = (rng.integers(70, 5000, int(spliced.sum())).astype(np.uint32) << 4) | 3
    rs = samio.ReadSet(pos, flag, off, cigar)
    xs = np.where(spliced, rng.choice(np.array([0, 43, 45], np.uint8), n), 0).astype(np.uint8)
    cover = _random_cover(rng, 1000, 3000000)
    want = S.tally(rs, xs, cover)
    assert want[0] == n and min(want) > 0
    assert _device_tally(ctx, rs, xs, cover) == want


# ---- content ------------------------------------------------------------------------------------------------------------------
def test_strand_bytes_without_a_map(ctx, content):
    rs, xs, _ = content
    want = S.tally(rs, xs, None)
    assert min(want[:8]) > 0 and not any(want[8:])
    assert _device_tally(ctx, rs, xs, None) == want


@pytest.mark.parametrize("n_cover", [1, 2, 3, 1000, 40000])
def test_a_map_without_strand_bytes_and_both_together(ctx, content, n_cover):
    rs, xs, covers = content
    cover = covers[n_cover]
    assert (n_cover > TOP) == (n_cover == 40000)
    want = S.tally(rs, None, cover)
    assert not any(want[2:8])
    assert _device_tally(ctx, rs, None, cover) == want
    both = S.tally(rs, xs, cover)
    assert both[8:] == want[8:] and both[:8] == S.tally(rs, xs, None)[:8]
    assert sum(both[8:]) > 100
    if n_cover >= 3:
        assert min(both[8:]) > 0
    assert _device_tally(ctx, rs, xs, cover) == both


def test_the_reads_in_any_order(ctx, content):
    rs, xs, covers = content
    perm = np.random.default_rng(5).permutation(rs.n)
    prs, pxs = _permuted(rs, xs, perm)
    assert not np.array_equal(prs.pos, rs.pos)
    for cover in (None, covers[1000], covers[40000]):
        want = S.tally(rs, xs, cover)
        assert S.tally(prs, pxs, cover) == want
        assert _device_tally(ctx, prs, pxs, cover) == want


def test_a_set_moved_into_a_shard_is_tallied_where_it_lies(ctx, content):
    """Map coordinates are the set's: a segment added with a shift meets the map moved by as much."""
    rs, xs, covers = content
    start, code = covers[1000]
    shift = 5000000
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, xs=xs)], with_strand=True) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0, shift)
            dr.finish()
            assert dr.strand_tally((start + shift, code)).tolist() == S.tally(rs, xs, (start, code))


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_working(ctx, content):
    rs, xs, covers = content
    arrays = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)
    dr = ctx.upload_reads(arrays)                  # (packed on the host: records, not arrays)
    try:
        with pytest.raises(native.SpliserNativeError, match="fused") as err:
            dr.strand_tally(covers[3])
        assert err.value.code == -1
    finally:
        dr.free()
    with ctx.upload_soa([arrays]) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            with pytest.raises(native.SpliserNativeError, match="nothing to tally") as err:
                dr.strand_tally(None)
            assert err.value.code == -1
            for bad in ((np.array([30, 20, 10], np.int32), np.array([1, 2, 1], np.uint8)), (np.array([10, 20, 20], np.int32), np.array([1, 2, 1], np.uint8))):
                with pytest.raises(native.SpliserNativeError, match="ascending") as err:
                    dr.strand_tally(bad)
                assert err.value.code == -1
            assert dr.strand_tally(covers[3]).tolist() == S.tally(rs, None, covers[3])
    assert _device_tally(ctx, rs, xs, covers[2]) == S.tally(rs, xs, covers[2])


# ---- the decodes --------------------------------------------------------------------------------------------------------------
NAMES, LENGTHS = ["c1", "c2", "c3"], [10 ** 6] * 3
SAM_TEXT = {X.TAG_KINDS[0][0]: "NH:i:1\tXS:A:+", X.TAG_KINDS[1][0]: "NH:i:1\tXS:A:-", X.TAG_KINDS[2][0]: "NH:i:1", X.TAG_KINDS[3][0]: "XS:i:37",
            X.TAG_KINDS[4][0]: "XS:i:43\tXS:A:-", X.TAG_KINDS[5][0]: "XS:A:.", X.TAG_KINDS[6][0]: "CO:Z:XSA+", X.TAG_KINDS[7][0]: "XS:A:+\tXS:A:-", b"": ""}


@pytest.fixture(scope="module")
def decode_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("sdec")
    rng = np.random.default_rng(31)
    sets = [(c, X.make_reads(rng, 1500)) for c in NAMES]
    tags, xs = zip(*[X.make_tags(rng, rs) for _, rs in sets])
    covers = {c: _random_cover(rng, n, 160000) for c, n in zip(NAMES, (40, 3000, 1))}
    bam, sam = str(d / "d.bam"), str(d / "d.sam")
    samio.write_bam(bam, NAMES, LENGTHS, sets, with_seq=True, unplaced=3, tags=list(tags))
    with open(sam, "w") as fh:
        fh.write("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in zip(NAMES, LENGTHS)))
        for (chrom, rs), tg in zip(sets, tags):
            for k in range(rs.n):
                cols = ["r", str(rs.flag[k]), chrom, str(rs.pos[k]), "60", samio.cigar_string(rs.cigar[rs.cig_off[k]:rs.cig_off[k + 1]]), "*", "0", "0", "*", "*"]
                fh.write("\t".join(cols + ([SAM_TEXT[tg[k]]] if SAM_TEXT[tg[k]] else [])) + "\n")
    want = {}
    for exclude in (0, 0x110):
        out = [0] * 14
        for (chrom, rs), x in zip(sets, xs):
            out = [a + b for a, b in zip(out, S.tally(rs, x, covers[chrom], keep=(rs.flag & exclude) == 0))]
        want[exclude] = out
    assert min(want[0]) > 0 and want[0x110][0] < want[0][0]
    return bam, sam, covers, want


@pytest.mark.parametrize("exclude", [0, 0x110])
@pytest.mark.parametrize("how", ["device", "host", "shares", "sam"])
def test_tally_after_every_decode(ctx, decode_files, how, exclude):
    bam_path, sam_path, covers, want = decode_files
    options = proc.DecodeOptions((0, 0, exclude), aux_strand=True)
    if how == "sam":
        source = proc.open_alignments(sam_path, options=options)
    else:
        source = native.BamFile(bam_path, threads=2, defer=True, exclude_flags=exclude, aux_strand=True)
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
            assert any(sum(1 for k in range(2) if source.share_ref(k, c)[0] > 0) == 2 for c in NAMES)      # (a chromosome is cut)
        assert sd.tally_of_source(source, devices, NAMES, covers).tolist() == want[exclude]
        one = sd.tally_of_source(source, devices, ["c2"], None)          # (-c, tags only)
        assert 0 < one[0] < want[exclude][0] and not one[8:].any()
    finally:
        if hasattr(source, "close"):
            source.close()


# ---- the commands -------------------------------------------------------------------------------------------------------------
LIBRARIES = {"fr": (1.0, 11), "rf": (0.0, 12), "unstranded": (0.5, 13), "undetermined": (0.75, 14)}


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("slib")
    gff, flipped = str(d / "genes.gff"), str(d / "flipped.gff")
    S.write_gff(gff)
    S.write_gff(flipped, flip=True)
    out = {"dir": str(d), "gff": gff, "flipped": flipped}
    for name, (p, seed) in LIBRARIES.items():
        sets, tags, xs = S.library(p, seed)
        path = str(d / (name + ".bam"))
        samio.write_bam(path, S.NAMES, S.LENGTHS, sets, with_seq=True, tags=tags)
        t = S.library_tally(sets, xs)
        # the yardstick's own verdict first: both sources have their 2000 reads and sit well inside the band
        for first in (2, 8):
            a, b = sum(t[first:first + 6:2]), sum(t[first + 1:first + 6:2])
            assert a + b >= 2000 and S.source_verdict(a, b) == name
            assert abs(10 * a - {"fr": 10, "rf": 0, "unstranded": 5, "undetermined": 7.5}[name] * (a + b)) <= 0.5 * (a + b)
        assert S.verdict(t) == name
        out[name] = (path, sets, xs, t)
    sets, tags, xs = S.library(1.0, 15, with_xs=False)
    path = str(d / "noxs.bam")
    samio.write_bam(path, S.NAMES, S.LENGTHS, sets, with_seq=True, tags=tags)
    out["noxs"] = (path, sets, xs, S.library_tally(sets, xs))
    return out


def _report_of(argv, path, capsys):
    assert cli.main(["strandedness", "-o", path] + argv) == 0
    text = open(path).read()
    log = capsys.readouterr().out
    assert all(line in log for line in text.splitlines())        # (the report is logged as well as written)
    return S.parse_report(text)


@pytest.mark.parametrize("name", list(LIBRARIES))
def test_strandedness_command_on_both_sources(libs, name, capsys):
    path, sets, xs, want = libs[name]
    got, per, final, notes = _report_of(["-B", path, "-A", libs["gff"]], libs["dir"] + "/%s.both.txt" % name, capsys)
    assert got == want and final == name and per["tags"][3] == per["annotation"][3] == name and not notes
    for source, first in (("tags", 2), ("annotation", 8)):
        a, b = sum(want[first:first + 6:2]), sum(want[first + 1:first + 6:2])
        assert per[source][:3] == (a, b, "%.4f" % (a / (a + b)))


def test_strandedness_command_what_it_writes_is_tally_of_source_and_the_decision(libs, capsys):
    path, _, _, want = libs["fr"]
    got, per, final, _ = _report_of(["-B", path, "-A", libs["gff"], "--hostDecode"], libs["dir"] + "/api.txt", capsys)
    from spliser_amd import sites
    bins = sites.GeneBins.from_annotation(libs["gff"], "gene", "All", log=lambda m: None)
    source = proc.open_and_decode(path, (0,), None, 0, proc.DecodeOptions(aux_strand=True))
    try:
        source.wait_all()
        t = sd.tally_of_source(source, (0,), S.NAMES, sd.covers_of(bins, S.NAMES))
    finally:
        source.close()
    assert t.tolist() == got == want and sd.decide(t)[0] == final == "fr"
    assert {k: v[3] for k, v in per.items()} == sd.decide(t)[1]


def test_strandedness_command_one_source_each_a_conflict_and_too_little(libs, capsys):
    d = libs["dir"]
    path, sets, xs, want = libs["rf"]
    got, per, final, _ = _report_of(["-B", path], d + "/tags.txt", capsys)                      # tags only
    assert got == S.library_tally(sets, xs, annotated=False) and final == "rf" and per["annotation"] == (0, 0, "NA", "none")
    path, sets, xs, want = libs["noxs"]                                                         # annotation only, and the hint
    got, per, final, notes = _report_of(["-B", path, "-A", libs["gff"]], d + "/ann.txt", capsys)
    assert got == want and final == "fr" and per["tags"] == (0, 0, "NA", "none") and notes == [sd.XS_HINT]
    path, sets, xs, _ = libs["fr"]                                                              # tags say fr, the flipped genes rf
    got, per, final, _ = _report_of(["-B", path, "-A", libs["flipped"]], d + "/conflict.txt", capsys)
    want = S.library_tally(sets, xs, flip=True)
    assert got == want and S.verdict(want) == final == "undetermined (tags and annotation disagree)"
    assert per["tags"][3] == "fr" and per["annotation"][3] == "rf"
    got, per, final, _ = _report_of(["-B", path, "-A", libs["gff"], "--minEvidence", "100000"], d + "/little.txt", capsys)
    assert final == S.verdict(got, 100000) == "undetermined (too little evidence)" and per["tags"][3] == per["annotation"][3] == "none"
    got, _, final, _ = _report_of(["-B", path, "-A", libs["gff"], "-c", "c2", "--excludeFlags", "0x10", "--minEvidence", "100"], d + "/c2.txt", capsys)
    keep = [(rs.flag & 0x10) == 0 for _, rs in sets]
    assert got == S.library_tally(sets[1:], xs[1:], keep=keep[1:]) and 100 <= sum(got[2:8]) < 1000 and final == S.verdict(got, 100) == "fr"


def _same_files(a, b, bed):
    assert open(a + ".SpliSER.tsv").read() == open(b + ".SpliSER.tsv").read()
    assert open(a + ".SpliSER.tsv").read().count("\n") > 20
    if bed:
        assert open(a + ".junctions.bed").read() == open(b + ".junctions.bed").read()


@pytest.mark.parametrize("mode", ["no_bed", "bed", "host_decode"])
@pytest.mark.parametrize("name", ["fr", "rf", "unstranded"])
def test_process_auto_writes_what_the_typed_verdict_writes(libs, name, mode, capsys):
    path, sets, xs, want = libs[name]
    d = libs["dir"]
    typed = [] if name == "unstranded" else ["--isStranded", "-s", name]
    extra = ["-A", libs["gff"]]
    if mode == "bed":
        bed = "%s/%s.in.bed" % (d, name)
        assert cli.main(["junctions", "-B", path, "-o", bed] + typed) == 0
        extra += ["-b", bed]
    else:
        extra += ["--keepJunctions"] + (["--hostDecode"] if mode == "host_decode" else [])
    a, b = "%s/%s.%s.auto" % (d, name, mode), "%s/%s.%s.typed" % (d, name, mode)
    capsys.readouterr()
    assert cli.main(["process", "-B", path, "-o", a, "-s", "auto"] + extra) == 0
    log = capsys.readouterr().out
    assert cli.main(["process", "-B", path, "-o", b] + typed + extra) == 0
    proc.wait_deferred_close()
    _same_files(a, b, mode != "bed")
    got, _, final, _ = S.parse_report(open(a + ".strandedness.txt").read())
    assert got == want and final == name and ("verdict\t" + name) in log
    assert not os.path.exists(b + ".strandedness.txt")
    if name != "unstranded" and mode != "bed":
        assert {"+", "-"} <= {line.split("\t")[2] for line in open(a + ".SpliSER.tsv").read().splitlines()[1:]}


def test_process_auto_without_a_verdict_is_an_error_that_leaves_nothing(libs, capsys):
    path = libs["undetermined"][0]
    out = libs["dir"] + "/undetermined.auto"
    with pytest.raises(sd.Undetermined) as err:
        cli.main(["process", "-B", path, "-o", out, "-s", "auto", "-A", libs["gff"], "--keepJunctions"])
    proc.wait_deferred_close()
    assert "verdict\tundetermined" in capsys.readouterr().out and "verdict\tundetermined" in err.value.report
    assert not os.path.exists(out + ".SpliSER.tsv") and not os.path.exists(out + ".junctions.bed")
    out = libs["dir"] + "/unstranded.isstranded"
    with pytest.raises(sd.Undetermined, match="unstranded"):
        cli.main(["process", "-B", libs["unstranded"][0], "-o", out, "--isStranded", "-s", "auto"])
    proc.wait_deferred_close()
    assert not os.path.exists(out + ".SpliSER.tsv")


def test_junctions_auto_writes_what_the_typed_verdict_writes(libs, capsys):
    d = libs["dir"]
    for name in ("rf", "unstranded"):
        a, b = "%s/%s.j.auto.bed" % (d, name), "%s/%s.j.typed.bed" % (d, name)
        assert cli.main(["junctions", "-B", libs[name][0], "-o", a, "-s", "auto"]) == 0
        assert ("verdict\t" + name) in capsys.readouterr().out
        assert cli.main(["junctions", "-B", libs[name][0], "-o", b] + ([] if name == "unstranded" else ["--isStranded", "-s", name])) == 0
        assert open(a).read() == open(b).read() and open(a).read().count("\n") > 20
