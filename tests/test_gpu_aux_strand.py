"""``--strandFromXS`` on the device: the strand byte the device extraction leaves per placed read against the host decoder's and
against what was written (both extraction kernels; the walking one is selected with SPL_EXTRACT_WALK=1, the switch of
tools/ingest_ab.py and the other decode tests -- no legal file overflows the scan's record list: SPL_BS_REC_CAP = 1824 places a
block, and a block of 65280 bytes holds at most 1764 records of the smallest legal size, 37 bytes); ``spl_junctions`` mode 3
on fused sets against the yardstick composed from ``oracle.junction_table`` (``xscases.yardstick``); the two commands."""
import struct
import zlib

import numpy as np
import pytest

import xscases as X
from spliser_amd import cli, junctions as jn, native, process as proc, samio, sites, tsv

pytestmark = pytest.mark.gpu

KNOBS = [(0, 0, 0), (8, 70, 500000)]
NAMES, LENGTHS = ["c1", "c2", "c3"], [10 ** 6] * 3
BLOCK = 0xFF00
XS3 = native.STRAND_FROM_XS


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


# ---- the file of the decode tests ------------------------------------------------------------------------------------------
def _record_size(serial, rs, k, tag):
    ops = rs.cigar[rs.cig_off[k]:rs.cig_off[k + 1]]
    qlen = int(sum(int(o) >> 4 for o in ops if (int(o) & 15) in (0, 1, 4, 7, 8)))
    return 4 + 32 + len("r%d" % serial) + 1 + 4 * len(ops) + (qlen + 1) // 2 + qlen + len(tag)


def _pad(n):
    """An aux field of exactly n >= 4 bytes."""
    return b"ZPZ" + b"p" * (n - 4) + b"\x00"


def _edge_file(path):
    """c1: random reads with every kind of tag, and wherever a BGZF block boundary comes near a spliced read that carries XS:A a pad
    field in front of the tag moves it so that the boundary cuts the field in two (tag | type and value).  c2: records of exactly
    1020 bytes, 64 to a block of 65280 whatever the offset.  c3: random again; five records without a reference at the end.
    -> (sets, tags, want, stream offsets of the XS:A fields that were moved onto a boundary)."""
    rng = np.random.default_rng(77)
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in zip(NAMES, LENGTHS))
    at = 4 + 4 + len(text) + 4 + sum(4 + len(n) + 1 + 4 for n in NAMES)
    sets, tags, cut = [], [], []
    serial = 0
    for chrom in NAMES:
        if chrom == "c2":
            rs = samio.ReadSet.from_records([(int(rng.choice([0, 16])), 1000 + 3 * i, "%dM%dN%dM" % (20 + i % 7, 100 + i % 5, 30)) for i in range(200)])
            t = []
            for k in range(rs.n):
                tail = [b"XSA+", b"XSA-", b"", b"XSi\x07\x00\x00\x00"][k % 4]
                t.append(_pad(1020 - _record_size(serial + k, rs, k, tail)) + tail)
                assert _record_size(serial + k, rs, k, t[-1]) == 1020
        else:
            rs = X.make_reads(rng, 1500, long_cigar_every=97)
            t, _ = X.make_tags(rng, rs)
            spliced = X.has_n(rs)
            o = at
            for k in range(rs.n):
                size = _record_size(serial + k, rs, k, t[k])
                where = t[k].find(b"XSA") if t[k].startswith(b"NHC") else -1      # (STAR's five: the field's place is known)
                boundary = (o // BLOCK + 1) * BLOCK
                xs_at = o + size - len(t[k]) + where
                if spliced[k] and where >= 0 and 4 <= boundary - 2 - xs_at < 200:
                    t[k] = t[k][:where] + _pad(boundary - 2 - xs_at) + t[k][where:]
                    cut.append(boundary - 2)
                    size = _record_size(serial + k, rs, k, t[k])
                o += size
        for k in range(rs.n):
            at += _record_size(serial + k, rs, k, t[k])
        serial += rs.n
        sets.append((chrom, rs))
        tags.append(t)
    samio.write_bam(path, NAMES, LENGTHS, sets, with_seq=True, unplaced=5, tags=tags)
    want = [X.expected_xs(rs, t) for (_, rs), t in zip(sets, tags)]
    return sets, tags, want, cut


def _inflate(path):
    data, out, at = open(path, "rb").read(), [], 0
    while at < len(data):
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        out.append(zlib.decompress(data[at + 18:at + bsize - 8], -15))
        at += bsize
    return out


@pytest.fixture(scope="module")
def edge_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("xs") / "edge.bam")
    sets, tags, want, cut = _edge_file(path)
    # the file is the case: the edges the issue names do occur in it
    blocks = _inflate(path)
    stream = b"".join(blocks)
    assert all(len(b) == BLOCK for b in blocks[:-2])
    assert len(cut) >= 3 and all(stream[o:o + 3] == b"XSA" and o // BLOCK != (o + 3) // BLOCK for o in cut)
    text_len = struct.unpack_from("<i", stream, 4)[0]
    at = 12 + text_len
    for _ in NAMES:
        at += 8 + struct.unpack_from("<i", stream, at)[0]
    per_block, tids = {}, {}
    while at < len(stream):
        bs, tid = struct.unpack_from("<ii", stream, at)
        per_block[at // BLOCK] = per_block.get(at // BLOCK, 0) + (tid >= 0)
        tids.setdefault(at // BLOCK, set()).add(tid)
        at += 4 + bs
    assert 64 in per_block.values() and max(per_block.values()) > 3 * 64
    assert any(len(t - {-1}) > 1 for t in tids.values()) and any(-1 in t for t in tids.values())
    return path, sets, tags, want


def _host(path, aux=True, **kw):
    bam = native.BamFile(path, threads=2, defer=True, **kw)
    if aux:
        bam.set_aux_strand(True)
    bam.start_host_decode()
    return bam


def _device(path, ctx, aux=True, **kw):
    bam = native.BamFile(path, threads=2, defer=True, **kw)
    if aux:
        bam.set_aux_strand(True)
    assert bam.decode_on_device(ctx) is True, bam.decline_reason()
    return bam


def _same_four(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("pos", "flag", "cig_off", "cigar"))


@pytest.mark.parametrize("walk", [False, True], ids=["wave", "walk"])
@pytest.mark.parametrize("window", [None, "3"], ids=["one_window", "windows_of_3"])
def test_device_decode_against_host_decode_against_what_was_written(edge_file, ctx, walk, window, monkeypatch):
    path, sets, tags, want = edge_file
    if walk:
        monkeypatch.setenv("SPL_EXTRACT_WALK", "1")
    if window:
        monkeypatch.setenv("SPL_INFLATE_WINDOW_BLOCKS", window)      # (records and their aux areas straddle the windows too)
    host, dev, plain = _host(path), _device(path, ctx), _device(path, ctx, aux=False)
    try:
        for (chrom, rs), w in zip(sets, want):
            with ctx.begin_reads() as dr:        # (asked where the arrays are: on the device)
                dr.add_bam(dev, chrom)
                dr.finish()
                assert dr.has_strand()
            with ctx.begin_reads() as dr:
                dr.add_bam(plain, chrom)
                dr.finish()
                assert not dr.has_strand()
                with pytest.raises(native.SpliserNativeError) as err:
                    dr.junctions(XS3)
                assert err.value.code == -1
            h, d, p = host.reads(chrom), dev.reads(chrom), plain.reads(chrom)
            assert np.array_equal(d.pos, rs.pos) and np.array_equal(d.flag, rs.flag) and np.array_equal(d.cigar, rs.cigar)
            assert _same_four(d, h) and _same_four(d, p), chrom
            assert p.xs is None
            assert np.array_equal(h.xs, w), chrom
            assert np.array_equal(d.xs, w), (chrom, np.flatnonzero(d.xs != w)[:10])
        assert dev.n_records == host.n_records == sum(rs.n for _, rs in sets) + 5
    finally:
        for b in (host, dev, plain):
            b.close()


def test_device_decode_under_a_read_filter(edge_file, ctx):
    path, sets, _, want = edge_file
    dev = _device(path, ctx, exclude_flags=0x110)
    try:
        for (chrom, rs), w in zip(sets, want):
            keep = (rs.flag & 0x110) == 0
            d = dev.reads(chrom)
            assert np.array_equal(d.pos, rs.pos[keep]) and np.array_equal(d.xs, w[keep])
    finally:
        dev.close()


def test_a_cg_tag_file_goes_to_the_host_and_carries_its_bytes(tmp_path, ctx):
    rng = np.random.default_rng(3)
    rs = X.make_reads(rng, 400)
    t, w = X.make_tags(rng, rs)
    path = str(tmp_path / "cg.bam")
    samio.write_bam(path, ["c"], [10 ** 6], [("c", rs)], long_cigar_tag=True, tags=[t])
    bam = native.BamFile(path, threads=2, defer=True)
    bam.set_aux_strand(True)
    assert bam.decode_on_device(ctx) is False and "CG" in bam.decline_reason()
    got = bam.reads("c")
    assert np.array_equal(got.cigar, rs.cigar) and np.array_equal(got.xs, w)
    bam.close()


# ---- spl_junctions, mode 3 ---------------------------------------------------------------------------------------------------
def _fused_rows(ctx, rs, xs, stranded, knobs, chunk=None):
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, xs=xs)], with_strand=xs is not None) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            assert dr.has_strand() == (xs is not None)
            rows = X.rows_of(dr.junctions(stranded, *knobs))
            assert dr.layout_bytes()[1] == 0          # (the set stays fused)
            return rows


def test_case_a_one_junction_three_rows(ctx):
    rs = samio.ReadSet.from_records([(0, 100, "20M100N30M"), (16, 105, "15M100N9M"), (0, 110, "10M100N40M"), (0, 112, "8M100N8M"),
                                     (0, 90, "30M100N12M"), (0, 100, "50M")])
    xs = np.array([43, 43, 45, 0, 0, 0], np.uint8)      # (+, +, -, untagged, XS:i, unspliced)
    assert _fused_rows(ctx, rs, xs, XS3, (0, 0, 0)) == [(119, 219, 43, 2, 20, 30), (119, 219, 45, 1, 10, 40), (119, 219, 63, 2, 30, 12)]
    for knobs in KNOBS + [(9, 70, 500000)]:
        assert _fused_rows(ctx, rs, xs, XS3, knobs) == X.yardstick(rs, xs, knobs)


def _case_b():
    """Tagged spliced reads on both sides of a tile boundary (256 reads) and of a chunk boundary (2048), between them a read whose
    CIGAR is longer than the 2048-word stage: 4200 reads at ascending positions."""
    recs, xs = [], []
    for i in range(4200):
        pos = 1000 + 10 * i
        if i in (255, 256, 257, 2047, 2048, 2049, 300, 2100) or i % 37 == 0:
            recs.append((16 if i % 2 else 0, pos, "%dM%dN%dM" % (10 + i % 9, 200 + (i % 3) * 50, 12 + i % 5)))
            xs.append([43, 45, 0][i % 3] if i not in (255, 257, 2047, 2049) else 43 if i < 1000 else 45)
        elif i in (1000, 2050):
            recs.append((0, pos, "1M1I" * 1100 + "5M300N7M"))       # 2203 ops: beyond the stage, read where it is
            xs.append(45 if i == 1000 else 0)
        else:
            recs.append((0, pos, "50M"))
            xs.append([0, 43][i % 2])           # (a byte on an unspliced read has nothing to say)
    return samio.ReadSet.from_records(recs), np.asarray(xs, np.uint8)


@pytest.mark.parametrize("knobs", KNOBS)
def test_case_b_tile_and_chunk_boundaries_and_a_read_beyond_the_stage(ctx, knobs):
    rs, xs = _case_b()
    want = X.yardstick(rs, xs, knobs)
    assert {r[2] for r in want} == {43, 45, 63}
    assert _fused_rows(ctx, rs, xs, XS3, knobs) == want


@pytest.mark.parametrize("knobs", KNOBS)
def test_case_c_host_decoded_arrays_and_modes_0_1_2_on_a_set_with_the_array(edge_file, ctx, knobs):
    path, sets, _, want = edge_file
    host = _host(path)
    try:
        for (chrom, rs), w in zip(sets, want):
            h = host.reads(chrom)
            rows = _fused_rows(ctx, h, h.xs, XS3, knobs)
            assert rows == X.yardstick(rs, w, knobs), chrom
            for mode in (0, 1, 2):          # (the fifth array changes nothing for who does not ask for it)
                assert _fused_rows(ctx, h, h.xs, mode, knobs) == _fused_rows(ctx, h, None, mode, knobs), (chrom, mode)
        assert len({r[2] for r in rows}) == 3
    finally:
        host.close()


def test_mode_3_without_the_array_or_on_a_set_that_is_not_fused_is_an_error(ctx):
    rs, xs = _case_b()
    with pytest.raises(native.SpliserNativeError, match="strand bytes") as err:
        _fused_rows(ctx, rs, None, XS3, (0, 0, 0))
    assert err.value.code == -1
    dr = ctx.upload_reads(native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar))
    try:
        assert not dr.has_strand()
        with pytest.raises(native.SpliserNativeError, match="fused") as err:
            dr.junctions(XS3)
        assert err.value.code == -1
        assert len(dr.junctions(0)["left"])           # (the context goes on)
    finally:
        dr.free()


@pytest.mark.parametrize("knobs", KNOBS)
def test_case_d_two_shares_on_two_contexts_merged(edge_file, knobs):
    path, sets, _, want = edge_file
    bam = native.BamFile(path, threads=2, defer=True)
    bam.set_aux_strand(True)
    try:
        bam.decode_on_devices_async([0, 0])
        assert bam.join_decoders() is True, bam.decline_reason()
        cut_somewhere = False
        got = jn.tables_of_source(bam, (0, 0), NAMES, XS3, *knobs)
        for (chrom, rs), w in zip(sets, want):
            cut_somewhere = cut_somewhere or sum(1 for k in range(2) if bam.share_ref(k, chrom)[0] > 0) == 2
            assert got[chrom][0] == rs.n and X.rows_of(got[chrom][1]) == X.yardstick(rs, w, knobs), chrom
        assert cut_somewhere
    finally:
        bam.close()


# ---- the commands -----------------------------------------------------------------------------------------------------------
def _expected_bed(sets, xs, knobs):
    text = [jn.track_line(*knobs)]
    n = 1
    import io
    for (chrom, rs), w in zip(sets, xs):
        buf = io.StringIO()
        n += jn.write_junction_bed(buf, chrom, X.table_of(X.yardstick(rs, w, knobs)), n)
        text.append(buf.getvalue())
    return "".join(text)


def _oracle_tsv(oracle_lib, bed, sets, chroms=None):
    """What tests/test_gpu_configs.py composes for a synthetic workload, for read sets: Steps 0-2 line by line, the oracle's counts."""
    table = sites.SiteTable(sites.GeneBins(), is_stranded=False)
    table.add_bed(bed, **({"q_chrom": chroms} if chroms else {}))
    table.find_competitors()
    text = [tsv.HEADER]
    by = dict(sets)
    for chrom in table.chrom_index:
        arr = table.chrom_arrays(chrom)
        if arr.n == 0:
            continue
        rd = by[chrom]
        cnt = oracle_lib.check_bam(arr.pos, arr.strand, arr.part_off, arr.part_pos, arr.comp_off, arr.comp_pos, rd.pos, rd.flag, rd.cig_off, rd.cigar, 0, 0)
        b2s, b2c, b2w, sse = oracle_lib.beta2_sse(arr.pos, arr.part_off, arr.part_pos, arr.part_site, arr.alpha, arr.edge_cnt, cnt[0], cnt[1], cnt[2], False)
        text.extend(tsv.format_chrom(arr, dict(beta1=cnt[0], beta2_simple=b2s, beta2_cryptic=b2c, beta2_weighted=b2w, sse=sse), False))
    return "".join(text)


@pytest.fixture(scope="module")
def command_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cmd")
    rng = np.random.default_rng(12)
    sets = [(c, X.make_reads(rng, 1200)) for c in NAMES]
    tags, want = zip(*[X.make_tags(rng, rs) for _, rs in sets])
    bam, sam = str(d / "m.bam"), str(d / "m.sam")
    samio.write_bam(bam, NAMES, LENGTHS, sets, with_seq=True, tags=list(tags))
    text = {X.TAG_KINDS[0][0]: "NH:i:1\tXS:A:+", X.TAG_KINDS[1][0]: "NH:i:1\tXS:A:-", X.TAG_KINDS[2][0]: "NH:i:1", X.TAG_KINDS[3][0]: "XS:i:37",
            X.TAG_KINDS[4][0]: "XS:i:43\tXS:A:-", X.TAG_KINDS[5][0]: "XS:A:.", X.TAG_KINDS[6][0]: "CO:Z:XSA+", X.TAG_KINDS[7][0]: "XS:A:+\tXS:A:-", b"": ""}
    with open(sam, "w") as fh:
        fh.write("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in zip(NAMES, LENGTHS)))
        for (chrom, rs), tg in zip(sets, tags):
            for k in range(rs.n):
                cols = ["r", str(rs.flag[k]), chrom, str(rs.pos[k]), "60", samio.cigar_string(rs.cigar[rs.cig_off[k]:rs.cig_off[k + 1]]), "*", "0", "0", "*", "*"]
                fh.write("\t".join(cols + ([text[tg[k]]] if text[tg[k]] else [])) + "\n")
    return bam, sam, sets, list(want), str(d)


@pytest.mark.parametrize("tag,source,pflags", [
    ("device", "bam", []), ("host", "bam", ["--hostDecode"]), ("shares", "bam", ["--devices", "0,0"]), ("chrom", "bam", ["-c", "c2"]), ("sam", "sam", []),
])
def test_one_command_writes_what_the_two_write_and_what_the_oracle_writes(tag, source, pflags, command_files, oracle_lib, capsys):
    bam, sam, sets, want, d = command_files
    src = bam if source == "bam" else sam
    knobs = (8, 70, 500000)
    bed, one, two = "%s/%s.bed" % (d, tag), "%s/%s.one" % (d, tag), "%s/%s.two" % (d, tag)
    jflags = [f for f in pflags if f != "--hostDecode"]
    assert cli.main(["junctions", "-B", src, "-o", bed, "--strandFromXS"] + jflags) == 0
    log = capsys.readouterr().out
    assert "strand from XS" in log
    chrom = pflags[pflags.index("-c") + 1] if "-c" in pflags else None
    kept = [(s, w) for s, w in zip(sets, want) if chrom in (None, s[0])]
    assert open(bed).read() == _expected_bed([s for s, _ in kept], [w for _, w in kept], knobs)
    assert cli.main(["process", "-B", src, "-b", bed, "-o", two] + pflags) == 0
    assert cli.main(["process", "-B", src, "-o", one, "--strandFromXS", "--keepJunctions"] + pflags) == 0
    got = open(one + ".SpliSER.tsv").read()
    assert got == open(two + ".SpliSER.tsv").read(), tag
    assert open(one + ".junctions.bed").read() == open(bed).read(), tag
    assert got == _oracle_tsv(oracle_lib, bed, sets, chrom), tag
    strands = {line.split("\t")[2] for line in got.splitlines()[1:]}
    assert {"+", "-"} <= strands and got.count("\n") > 50, strands


def test_without_the_flag_the_file_is_the_all_question_mark_file(command_files, oracle_lib):
    bam, _, sets, _, d = command_files
    knobs = (8, 70, 500000)
    out, bed = d + "/plain", d + "/plain.mode0.bed"
    assert cli.main(["process", "-B", bam, "-o", out, "--keepJunctions"]) == 0
    with open(bed, "w") as fh:       # (the parent's path: mode 0, whose yardstick is the oracle's own table)
        fh.write(_expected_bed([s for s in sets], [np.zeros(rs.n, np.uint8) for _, rs in sets], knobs))
    assert open(out + ".junctions.bed").read() == open(bed).read()
    got = open(out + ".SpliSER.tsv").read()
    assert got == _oracle_tsv(oracle_lib, bed, sets)
    assert {line.split("\t")[2] for line in got.splitlines()[1:]} == {"?"}
