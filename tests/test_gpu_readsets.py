"""``readsets`` on the device: the one plan, after every kind of decode -- whole on the device, by the host's threads, in two shares,
by the Python reader from SAM text --, hands every read of a small file to its visitor exactly once, in fused sets that have the
strand bytes and name keys the source was opened for; and the set the plan hands out is the set the four consumers built on it see:
what ``gene_counts``, ``strand_tally``, ``junctions`` and ``coverage`` give in one visit is what ``genecounts.counts_of_source``,
``strandedness.tally_of_source``, ``junctions.tables_of_source`` and ``coverage.runs_of_source`` return for the same source."""
import threading

import numpy as np
import pytest

from spliser_amd import coverage as cov, genecounts as gc, junctions as jn, native, process as proc, readsets, samio, strandedness as sd

pytestmark = pytest.mark.gpu

NAMES, LENGTHS = ["c1", "c2", "c3"], [10 ** 6] * 3
PER = 100          # reads a reference.  300 reads of 1500 bases are eleven BGZF blocks: the share planner cuts a file of fewer than
#                    eight blocks into one share only, and two equal shares of this one cut c2
ONE = "c2"         # the chromosome whose set goes through all four consumers
N_GENES = 3
KNOBS = (8, 70, 500000)


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Per reference ``PER`` reads in turn plain, spliced with an XS:A tag (+ and - alternate), first of a pair, second of that pair
    (the same name; the mates overlap) -> paths of the BAM and of its SAM text."""
    d = tmp_path_factory.mktemp("readsets")
    sets, tags, names = [], [], []
    for chrom in NAMES:
        recs, t, nm = [], [], []
        for k in range(PER):
            kind, pos = k % 4, 100 + 40 * k
            recs.append(((0, 16 * (k // 4 % 2), 97, 145)[kind], pos, "700M300N800M" if kind == 1 else "1500M"))
            t.append((b"XSA+", b"XSA-")[k // 4 % 2] if kind == 1 else b"")
            nm.append(("%s_p%d" % (chrom, k - (kind == 3)) if kind >= 2 else "%s_r%d" % (chrom, k)).encode("ascii"))
        sets.append((chrom, samio.ReadSet.from_records(recs)))
        tags.append(t)
        names.append(nm)
    bam, sam = str(d / "r.bam"), str(d / "r.sam")
    samio.write_bam(bam, NAMES, LENGTHS, sets, with_seq=True, unplaced=3, tags=tags, names=names)
    with open(sam, "w") as fh:
        fh.write("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in zip(NAMES, LENGTHS)))
        for (chrom, rs), t, nm in zip(sets, tags, names):
            for k in range(rs.n):
                cols = [nm[k].decode("ascii"), str(rs.flag[k]), chrom, str(rs.pos[k]), "60", samio.cigar_string(rs.cigar[rs.cig_off[k]:rs.cig_off[k + 1]]), "*", "0", "0", "*", "*"]
                fh.write("\t".join(cols + (["XS:A:" + chr(t[k][3])] if t[k] else [])) + "\n")
    return dict(bam=bam, sam=sam)


def _open(files, ctx, how, options):
    """-> (source, devices) after the decode ``how``."""
    if how == "sam":
        return proc.open_alignments(files["sam"], options=options), (0,)
    source = native.BamFile(files["bam"], threads=2, defer=True, aux_strand=options.aux_strand, mate_keys=options.mate_keys)
    try:
        if how == "device":
            assert source.decode_on_device(ctx) is True, source.decline_reason()
        elif how == "host":
            source.start_host_decode()
        else:
            source.decode_on_devices_async([0, 0])
            assert source.join_decoders() is True, source.decline_reason()
            assert len(source.shares) == 2
            assert any(sum(1 for k in range(2) if source.share_ref(k, c)[0] > 0) == 2 for c in NAMES)      # (a chromosome is cut)
    except BaseException:
        source.close()
        raise
    return source, ((0, 0) if how == "shares" else (0,))


def _maps():
    """Three genes on ``ONE``, apart: under its first reads, its middle ones and its last ones."""
    left, right = np.array([100, 3000, 5300], np.int64), np.array([2000, 3600, 7000], np.int64)
    return {ONE: gc.gene_maps(left, right, np.array([43, 45, 43], np.uint8), np.arange(3), stranded=False)}


def _same_table(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("with_extras", [True, False])
@pytest.mark.parametrize("how", ["device", "host", "shares", "sam"])
def test_every_read_once_in_fused_sets_with_what_the_source_was_opened_for(files, ctx, how, with_extras):
    options = proc.DecodeOptions(aux_strand=with_extras, mate_keys=with_extras)
    source, devices = _open(files, ctx, how, options)
    seen, lock = [], threading.Lock()

    def visit(dr, chrom):
        row = (chrom, dr.n, dr.has_strand(), dr.has_mate_keys())
        with lock:
            seen.append(row)
    try:
        readsets.over_fused_sets(source, devices, NAMES, visit, with_keys=with_extras, with_strand=with_extras)
        one = []
        readsets.over_fused_sets(source, devices, [ONE], lambda dr, chrom: one.append((chrom, dr.n)))          # (-c)
    finally:
        if hasattr(source, "close"):
            source.close()
    assert {c: sum(n for chrom, n, _, _ in seen if chrom == c) for c in NAMES} == dict.fromkeys(NAMES, PER)
    assert len(seen) == (4 if how == "shares" else 3)                    # (two shares: two references whole, one in two pieces)
    assert {(s, k) for _, _, s, k in seen} == {(with_extras, with_extras)}
    assert {c for c, _ in one} == {ONE} and sum(n for _, n in one) == PER


@pytest.mark.parametrize("how", ["device", "host", "sam"])
def test_one_set_through_all_four_consumers_is_what_their_functions_return(files, ctx, how):
    source, devices = _open(files, ctx, how, proc.DecodeOptions(aux_strand=True, mate_keys=True))
    maps, got = _maps(), {}

    def visit(dr, chrom):
        length = LENGTHS[NAMES.index(chrom)] if how != "sam" else int(source.reads(chrom).max_end)      # (``coverage``'s rule: the header's, else the reads')
        got["genes"] = dr.gene_counts(N_GENES, *maps[chrom], 0, fragments=True)
        got["tally"] = dr.strand_tally(None)
        got["junctions"] = {mode: dr.junctions(mode, *KNOBS) for mode in (0, native.STRAND_FROM_XS)}
        got["coverage"] = (length, dr.coverage(length, 0, 0, fragments=True))
    try:
        readsets.over_fused_sets(source, devices, [ONE], visit, with_keys=True, with_strand=True)
        assert int(got["genes"].sum()) == PER - PER // 4 and got["genes"][:N_GENES].all()             # (a pair counts once; every gene has reads)
        assert gc.counts_of_source(source, devices, [ONE], maps, N_GENES, 0, fragments=True).tolist() == got["genes"].tolist()
        assert got["tally"][0] == PER and got["tally"][2:8].any()
        assert sd.tally_of_source(source, devices, [ONE], None).tolist() == got["tally"].tolist()
        for mode, want in got["junctions"].items():          # (mode 0 of reads on the host is ``junctions``' own, unfused path)
            n, table = jn.tables_of_source(source, devices, [ONE], mode, *KNOBS)[ONE]
            assert n == PER and _same_table(table, want) and int(table["count"].sum()) == PER // 4, mode
        assert set(got["junctions"][native.STRAND_FROM_XS]["strand"].tolist()) == {43, 45}
        (chrom, length, (track,)), = list(cov.runs_of_source(source, 0, [ONE], 0, fragments=True))
        want_length, (start, end, depth, totals) = got["coverage"]
        assert (chrom, length) == (ONE, want_length) and totals["pairs"] == PER // 4
        assert all(np.array_equal(a, b) for a, b in zip(track[:3], (start, end, depth))) and track[3] == totals
    finally:
        if hasattr(source, "close"):
            source.close()
