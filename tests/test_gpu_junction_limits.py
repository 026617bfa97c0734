"""The junction table on the device (spl_junction_kernel + spl_junction_compact_kernel through spl_junctions) against its
plain-Python restatement, oracle.junction_table, on the cases of junctioncases.py: the whole table -- left, right, strand, count,
both anchors -- for every strand mode and every filter setting the case names, at both chunk sizes, from every way a read set
is made (host packer, segments with shifts, BAM-native arrays fused and laid out, a BAM decoded on the device, the shares of a
decode in shares); then the `junctions` command's BED12 file and `process --checkJunctions`' table, byte for byte / row for
row, on one device and on several contexts."""
import io

import numpy as np
import pytest

import junctioncases as J
import limitcases as L
from oracle import oracle
from spliser_amd import cli, junctions as jn, native, process as proc

pytestmark = pytest.mark.gpu

CHUNKS = (J.CHUNK, J.CHUNK_BIG)


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


class Wants(object):
    """oracle.junction_table of a case, per (stranded, a, m, M), computed once."""

    def __init__(self, case):
        self.case, self.memo = case, {}

    def __call__(self, stranded, a, m, mx):
        k = (stranded, a, m, mx)
        if k not in self.memo:
            self.memo[k] = self.case.want(stranded, a, m, mx)
        return self.memo[k]


def _check_all(dr, case, want, tag):
    for stranded in (0, 1, 2):
        for a, m, mx in case.filters:
            got = J.rows(dr.junctions(stranded, a, m, mx))
            assert got == want(stranded, a, m, mx), tag + ("stranded", stranded, "filter", (a, m, mx))


def _table_for(case):
    """A site table over the case's junctions (rows at both ends, partners linked, a few rivals) for the counting pass that
    follows a junction table on the same read set."""
    tb = L.TableBuilder(len(case.name))
    js = [w for w in case.want(0, 0, 0, 0) if w[0] >= 0][:150]
    rows = {}

    def row(x, k):
        if x not in rows:
            rows[x] = tb.row(x, "+-"[k % 2])
        return rows[x]
    for k, (l, r, *_rest) in enumerate(js):
        tb.link(row(l, k), row(r, k + 1))
    for k in range(1, len(js) - 1, 3):
        tb.rival(rows[js[k][1]], rows[js[k - 1][0]], js[k + 1][1])
    if not rows:
        tb.row(100, "+")
    return tb.build()


def _count_and_check(ctx, oracle_lib, dr, table, reads, tag):
    """count_launch + SSE on a read set the junction table has just unfused: counters and SSE equal to the oracle's."""
    with ctx.upload_sites(table.sites()) as ds:
        for stranded in (0, 1):
            want = oracle_lib.check_bam(table.pos, table.strand, table.part_off, table.part_pos, table.comp_off, table.comp_pos,
                                        reads.pos, reads.flag, reads.cig_off, reads.cigar, stranded, 0)
            ctx.count_launch(ds, dr, stranded, 0)
            got = ds.counters()
            for w, g in zip(want, got):
                assert np.array_equal(w, g), tag + ("counters", stranded)
            ctx.sse_launch(ds, bool(stranded))
            want_sse = oracle_lib.beta2_sse(table.pos, table.part_off, table.part_pos, table.part_site, table.alpha, table.edge_cnt,
                                            want[0], want[1], want[2], bool(stranded))
            for w, g in zip(want_sse, ds.sse_results()):
                assert np.array_equal(np.asarray(g), np.asarray(w), equal_nan=w.dtype.kind == "f"), tag + ("sse", stranded)


# ---- every case, every way a read set is made ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", J.CASE_NAMES)
def test_junction_table_matches_restatement(name, ctx, oracle_lib, monkeypatch):
    case = J.case(name)
    want = Wants(case)
    table = _table_for(case) if case.reads.n else None
    for chunk in CHUNKS:
        monkeypatch.setenv("SPL_FORCE_CHUNK", str(chunk))
        # the host packer, the whole set at once (segments already moved)
        r = case.reads
        dr = ctx.upload_reads(native.ReadArrays(r.pos, r.flag, r.cig_off, r.cigar))
        try:
            _check_all(dr, case, want, (name, "upload_reads", chunk))
        finally:
            dr.free()
        # segment by segment with their shifts: the table comes back in the moved coordinates
        with ctx.begin_reads() as dr:
            for rs, shift in case.segments:
                dr.add(native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar), shift)
            dr.finish()
            _check_all(dr, case, want, (name, "add", chunk))
        # BAM-native arrays on the device: fused (the junction table lays the set out first) and laid out at finish
        for fused in (0, 1):
            monkeypatch.setenv("SPL_FUSED", str(fused))
            with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar) for rs, _ in case.segments]) as soa:
                with ctx.begin_reads() as dr:
                    for k, (_, shift) in enumerate(case.segments):
                        dr.add_soa(soa, k, shift)
                    dr.finish()
                    tag = (name, "soa", chunk, "fused", fused)
                    if case.reads.n:
                        assert (dr.layout_bytes()[1] == 0) == bool(fused), tag
                    _check_all(dr, case, want, tag)
                    if table is not None:
                        _count_and_check(ctx, oracle_lib, dr, table, case.reads, tag)
            monkeypatch.delenv("SPL_FUSED")


def test_read_past_coord_max_is_refused_and_the_context_recovers(ctx, monkeypatch):
    bad = J.beyond_coord_max()
    good = J.filter_boundaries_case()
    want = Wants(good)
    for fused in (0, 1):
        monkeypatch.setenv("SPL_FUSED", str(fused))
        dr = ctx.upload_reads(native.ReadArrays(bad.pos, bad.flag, bad.cig_off, bad.cigar))
        try:
            with pytest.raises(native.SpliserNativeError) as err:
                dr.junctions(0)
            assert err.value.code == -6
        finally:
            dr.free()
        with ctx.upload_soa([native.ReadArrays(bad.pos, bad.flag, bad.cig_off, bad.cigar)]) as soa:
            with ctx.begin_reads() as dr:
                dr.add_soa(soa, 0, 0)
                dr.finish()
                with pytest.raises(native.SpliserNativeError) as err:
                    dr.junctions(1, 0, 0, 0)
                assert err.value.code == -6
        # the same context, the next set: as if nothing had happened
        r = good.reads
        dr = ctx.upload_reads(native.ReadArrays(r.pos, r.flag, r.cig_off, r.cigar))
        try:
            _check_all(dr, good, want, ("after the range error", fused))
        finally:
            dr.free()
    # a set that ends exactly at SPL_COORD_MAX is no error
    top = J.coordinates_case()
    dr = ctx.upload_reads(native.ReadArrays(top.reads.pos, top.reads.flag, top.reads.cig_off, top.reads.cigar))
    try:
        _check_all(dr, top, Wants(top), ("coordinates",))
    finally:
        dr.free()


# ---- BAM files decoded on the device -------------------------------------------------------------------------------------------

def _sorted(recs):
    """Placed reads in POS order: what a sorted BAM file holds (a POS of 0 is an unplaced record there)."""
    return sorted((r for r in recs if r[1] > 0), key=lambda r: r[1])


def _bam_cases():
    """What goes into the BAM file of the tests below, one reference each (sorted by POS; the coordinates case stays out: a
    reference of 2^31 bases is more than a header's length field holds)."""
    return [J.case(n) for n in ("record_classes", "filter_boundaries", "wave_merge", "hash", "shifted_segments", "many_chunks")]


@pytest.fixture(scope="module")
def bam_file(tmp_path_factory):
    cases = _bam_cases()
    names = ["r_%s" % c.name for c in cases]
    sets = [L.reads_from(_sorted(c.recs)) for c in cases]
    path = str(tmp_path_factory.mktemp("jbam") / "j.bam")
    native.write_bam(path, names, [1 << 30] * len(names), sets, level=1, threads=2, seq_mode=1)
    return path, names, cases, sets


def _case_of_set(case, rs):
    return J.JCase(case.name, [(rs, 0)], case.filters, case.limit)


def test_device_decoded_bam(ctx, oracle_lib, bam_file, monkeypatch):
    path, names, cases, sets = bam_file
    for chunk in CHUNKS:
        monkeypatch.setenv("SPL_FORCE_CHUNK", str(chunk))
        for fused in (0, 1):
            monkeypatch.setenv("SPL_FUSED", str(fused))
            bam = native.BamFile(path, threads=2, defer=True)
            try:
                assert bam.decode_on_device(ctx), bam.decline_reason()
                for name, case, rs in zip(names, cases, sets):
                    c = _case_of_set(case, rs)
                    with ctx.begin_reads() as dr:
                        assert dr.add_bam(bam, name) == rs.n
                        dr.finish()
                        tag = (case.name, "add_bam", chunk, "fused", fused)
                        assert (dr.layout_bytes()[1] == 0) == bool(fused), tag
                        _check_all(dr, c, Wants(c), tag)
                        if fused and case.name in ("filter_boundaries", "hash", "shifted_segments"):
                            _count_and_check(ctx, oracle_lib, dr, _table_for(c), c.reads, tag)
            finally:
                bam.close()


def _share_holdings(path, names):
    """Reads of each reference in each share of a decode in three shares on device 0."""
    bam = native.BamFile(path, threads=2, stream=True, defer=True)
    try:
        bam.decode_on_devices_async([0, 0, 0])
        assert bam.join_decoders()
        return bam, [[bam.share_ref(k, c)[0] for c in names] for k in range(len(bam.shares))]
    except BaseException:
        bam.close()
        raise


def test_shares_of_a_device_decode(ctx, bam_file):
    """add_bam_share of every share: the per-share tables, merged by key (counts added, anchors the maximum), are the table of the
    whole reference."""
    path, names, cases, sets = bam_file
    bam, held = _share_holdings(path, names)
    try:
        held = np.array(held)
        assert held.shape[0] == 3 and held.sum(axis=0).tolist() == [rs.n for rs in sets]
        assert np.any((held > 0).sum(axis=0) > 1)                     # a reference IS cut across shares
        for j, (name, case, rs) in enumerate(zip(names, cases, sets)):
            c = _case_of_set(case, rs)
            for stranded in (0, 1, 2):
                for a, m, mx in c.filters:
                    parts = []
                    for k in range(3):
                        with ctx.begin_reads() as dr:
                            if dr.add_bam_share(bam, k, name) == 0:
                                continue
                            dr.finish()
                            parts.append(dr.junctions(stranded, a, m, mx))
                    assert J.merge_tables(parts) == c.want(stranded, a, m, mx), (name, stranded, (a, m, mx))
    finally:
        bam.close()


# ---- the `junctions` command and `process --checkJunctions` ---------------------------------------------------------------------

def _same_text(got, want):
    """got == want, and where not, the first line that differs (a diff of the whole files takes minutes)."""
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        k = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        raise AssertionError("line %d of %d / %d: %r != %r" % (k, len(g), len(w), g[k] if k < len(g) else None, w[k] if k < len(w) else None))


def _table_dict(rows):
    cols = list(zip(*rows)) if rows else [()] * 6
    dt = (np.int32, np.int32, np.uint8, np.uint32, np.uint32, np.uint32)
    return {k: np.array(v, d) for k, v, d in zip(("left", "right", "strand", "count", "anchor_left", "anchor_right"), cols, dt)}


def _expected_bed(names, sets, stranded, a, m, mx, only=None):
    out = io.StringIO()
    out.write('track name=junctions description="spliser_amd junctions (a>=%d, %d<=intron<=%d)"\n' % (a, m, mx))
    total = 0
    for name, rs in zip(names, sets):
        if only is not None and name != only:
            continue
        rows = oracle.junction_table(rs.pos, rs.flag, rs.cig_off, rs.cigar, stranded, a, m, mx)
        total += jn.write_junction_bed(out, name, _table_dict(rows), total + 1)
    return out.getvalue()


@pytest.mark.parametrize("argv,stranded,knobs,only", [
    ([], 0, J.DEFAULTS, None),
    (["-a", "1", "-m", "1", "-M", "0"], 0, (1, 1, 0), None),
    (["--isStranded", "-s", "fr"], 1, J.DEFAULTS, None),
    (["--isStranded", "-s", "rf", "-a", "0", "-m", "0", "-M", "0"], 2, (0, 0, 0), None),
    (["-c", "r_filter_boundaries", "-a", "10", "-m", "100", "-M", "100"], 0, (10, 100, 100), "r_filter_boundaries"),
    (["--devices", "0,0,0"], 0, J.DEFAULTS, None),
    (["--devices", "0,0,0", "--isStranded", "-s", "fr", "-a", "1", "-m", "0", "-M", "0"], 1, (1, 0, 0), None),
])
def test_junctions_command_writes_the_restated_bed(argv, stranded, knobs, only, bam_file, tmp_path):
    path, names, cases, sets = bam_file
    if "--devices" in argv:
        bam, held = _share_holdings(path, names)
        bam.close()
        assert any(sum(1 for k in range(len(held)) if held[k][j] > 0) > 1 for j in range(len(names)))   # a reference is cut
    out = str(tmp_path / "j.bed")
    assert cli.main(["junctions", "-B", path, "-o", out] + argv) == 0
    _same_text(open(out).read(), _expected_bed(names, sets, stranded, *knobs, only=only))


@pytest.mark.parametrize("devices", ["0", "0,0"])
@pytest.mark.parametrize("stranded", [None, "fr"])
def test_process_check_junctions(devices, stranded, bam_file, tmp_path):
    path, names, cases, sets = bam_file
    scode = native.STRANDED_CODE[stranded]
    bed = str(tmp_path / "s.bed")
    with open(bed, "w") as fh:
        fh.write(_expected_bed(names, sets, scode, *J.DEFAULTS))
    flags = ["--isStranded", "-s", stranded] if stranded else []
    base = ["process", "-B", path, "-b", bed, "--devices", devices] + flags
    plain, checked = str(tmp_path / "plain"), str(tmp_path / "checked")
    assert cli.main(base + ["-o", plain]) == 0
    assert cli.main(base + ["-o", checked, "--checkJunctions"]) == 0
    assert open(checked + ".SpliSER.tsv", "rb").read() == open(plain + ".SpliSER.tsv", "rb").read()
    table = proc._site_table(bed, "All", "All", 0, None, "gene", bool(stranded), stranded, lambda m: None)
    want = []
    for chrom in table.chrom_index:
        arr = table.chrom_arrays(chrom)
        if arr.n == 0:
            continue
        rs = sets[names.index(chrom)]
        rows = oracle.junction_table(rs.pos, rs.flag, rs.cig_off, rs.cigar, scode)
        want += [(chrom,) + tuple(r) for r in proc.junction_consistency(arr, _table_dict(rows), 0, bool(stranded))]
    with open(checked + ".junctionCheck.tsv") as fh:
        head = fh.readline()
        got = [line.rstrip("\n").split("\t") for line in fh]
    assert head.startswith("Region\tLeft\tRight\tStrand\tBED_alpha\tBAM_reads")
    got = [(g[0], int(g[1]), int(g[2]), g[3], int(g[4]), int(g[5])) for g in got]
    assert len(got) == len(want) and next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), None) is None
    assert len(want) > 0 and any(w[4] < w[5] for w in want) and any(w[4] == 0 for w in want)
