"""``--anyOrder`` (``spl_bam_set_any_order``) without a GPU: the host decoder under the switch on files whose records come in any
order, against numpy's stable sort of the records that were written (``ordercases``), and the switch's rules.  The reference has no
counterpart: it reads through ``samtools view BAM region`` (SpliSER_v0_1_8.py:422) and needs ``samtools sort`` first."""
import numpy as np
import pytest

import ordercases as O
import xscases as X
from spliser_amd import cli, native, synth


@pytest.fixture(scope="module", autouse=True)
def _built():
    native.build()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Five references, the reads of a small workload: in coordinate order and shuffled by a seed."""
    d = tmp_path_factory.mktemp("anyorder")
    wl = synth.Workload("arabidopsis", scale=0.002, seed=3, workers=2)
    a, b = str(d / "sorted.bam"), str(d / "shuffled.bam")
    mixed = O.shuffle_workload(wl, a, b, seed=41)
    return wl, a, b, mixed


def _host(path, **kw):
    bam = native.BamFile(path, threads=3, defer=True, **kw)
    bam.start_host_decode()
    return bam


def test_a_shuffled_file_under_the_switch(files):
    wl, a, b, mixed = files
    names = wl.genome.chrom_names
    want = O.expected(mixed, len(names))
    on, srt = _host(b, any_order=True), _host(a)
    assert on.wait_all() is True
    assert on.decline_reason() == ""
    n_sorted, on_gpu = on.any_order_sorted()
    assert n_sorted == sum(rs.n for rs in wl.reads) and on_gpu is False
    for tid, name in enumerate(names):
        got = on.reads(name)
        assert O.same_reads(got, want[tid][0]), name          # POS non-decreasing, ties in file order: numpy's stable sort
        assert np.all(np.diff(got.pos.astype(np.int64)) >= 0)
        assert O.multiset(got) == O.multiset(srt.reads(name)) == O.multiset(wl.reads[tid])
        assert on.wait_ref(name) == (wl.reads[tid].n, srt.wait_ref(name)[1])
    on.close()
    srt.close()


def test_the_same_file_without_the_switch(files):
    wl, a, b, mixed = files
    off = _host(b)
    assert off.wait_all() is False
    want = O.expected(mixed, 5, any_order=False)       # (file order within a reference: as before)
    for tid, name in enumerate(wl.genome.chrom_names):
        assert O.same_reads(off.reads(name), want[tid][0]), name
    assert off.any_order_sorted() == (0, False)
    off.close()


def test_a_sorted_file_is_left_as_it_is(files):
    wl, a, b, mixed = files
    on, off = _host(a, any_order=True), _host(a)
    assert on.wait_all() is True and off.wait_all() is True
    assert on.any_order_sorted() == (0, False)
    for name in wl.genome.chrom_names:
        x, y = on.reads(name), off.reads(name)
        for f in ("pos", "flag", "cig_off", "cigar"):
            assert getattr(x, f).tobytes() == getattr(y, f).tobytes(), (name, f)
        assert x.max_end == y.max_end
    on.close()
    off.close()


def test_sorted_by_reference_but_not_by_position_stays(tmp_path):
    """Reference ids never go down, POS does inside a reference: accepted without the switch, and left alone under it."""
    recs = [(0, 50, 0, 60, [(30 << 4)], b""), (0, 10, 16, 60, [(20 << 4)], b""), (1, 7, 0, 60, [(5 << 4)], b""), (1, 3, 0, 60, [(9 << 4)], b"")]
    path = str(tmp_path / "p.bam")
    O.write_bam(path, ["a", "b"], [1000, 1000], recs)
    on = _host(path, any_order=True)
    assert on.wait_all() is True and on.any_order_sorted() == (0, False)
    assert on.reads("a").pos.tolist() == [50, 10] and on.reads("b").pos.tolist() == [7, 3]
    on.close()


def test_the_switch_only_before_the_decode(files):
    wl, a, b, mixed = files
    bam = native.BamFile(b, threads=2, defer=True)
    bam.set_any_order(True)
    bam.set_any_order(False)
    bam.set_any_order(True)
    bam.start_host_decode()
    with pytest.raises(native.SpliserNativeError) as e:
        bam.set_any_order(False)
    assert "being decoded" in str(e.value)
    assert bam.wait_all() is True
    with pytest.raises(native.SpliserNativeError):
        bam.set_any_order(True)
    bam.close()
    with pytest.raises(native.SpliserNativeError):      # (shares are cut on the order of references)
        late = native.BamFile(b, threads=2, defer=True, any_order=True)
        try:
            late.decode_on_devices_async([0, 1])
        finally:
            late.close()


def test_strand_bytes_flags_and_empty_cigars_travel_with_their_reads(tmp_path):
    """XS-tagged spliced reads (the records of xscases) on two references, reads without a CIGAR and unmapped-but-placed reads among
    them, records without a reference in between, a reference with no reads; under a read filter as well."""
    rng = np.random.default_rng(8)
    sets, tags = [], []
    for _ in range(2):
        rs = X.make_reads(rng, 400)
        t, _ = X.make_tags(rng, rs)
        sets.append(rs)
        tags.append(t)
    recs = O.records_of([sets[0], None, sets[1]], tags=[tags[0], None, tags[1]], mapq=[rng.integers(0, 61, 400), None, rng.integers(0, 61, 400)])
    recs += [(0, 77, 0, 60, [], b""), (2, 5, 4, 0, [], b""), (-1, 0, 4, 0, [], b""), (-1, 0, 4, 0, [], b"")]       # '*' CIGARs, no reference
    mixed = O.shuffled(recs, 12)
    path = str(tmp_path / "x.bam")
    O.write_bam(path, ["a", "empty", "b"], [10 ** 6] * 3, mixed)
    for filt in ((0, 0, 0), (10, 0, 0x100)):
        want = O.expected(mixed, 3, filt)
        on = _host(path, any_order=True, aux_strand=True, min_mapq=filt[0], require_flags=filt[1], exclude_flags=filt[2])
        assert on.wait_all() is True
        for tid, name in enumerate(["a", "empty", "b"]):
            got = on.reads(name)
            assert O.same_reads(got, want[tid][0]), (name, filt)
            if want[tid][0].n:
                assert np.array_equal(got.xs, X.expected_xs(want[tid][0], want[tid][1])), (name, filt)
        assert on.reads("empty").n == 0
        on.close()


def test_the_flag_on_the_command_line(files, tmp_path, capsys):
    wl, a, b, mixed = files
    p = cli.build_parser()
    assert p.parse_args(["process", "-B", "x.bam", "-o", "o", "--anyOrder"]).anyOrder is True
    assert p.parse_args(["process", "-B", "x.bam", "-b", "x.bed", "-o", "o"]).anyOrder is False
    assert p.parse_args(["junctions", "-B", "x.bam", "-o", "o", "--anyOrder"]).anyOrder is True
    assert p.parse_args(["flagstat", "-B", "x.bam", "-o", "o", "--anyOrder"]).anyOrder is True
    for command in ("combine", "combineShallow"):
        with pytest.raises(SystemExit):
            p.parse_args([command, "-S", "s.tsv", "-o", "o", "--anyOrder"])
    capsys.readouterr()
    # flagstat on host threads: the same lines for the two files, and the line that says what happened for the shuffled one only
    assert cli.main(["flagstat", "-B", b, "-o", str(tmp_path / "b.txt"), "--hostDecode", "--anyOrder", "--threads", "2"]) == 0
    out = capsys.readouterr().out
    assert "the alignment file is not in coordinate order: %d reads sorted on host threads" % sum(rs.n for rs in wl.reads) in out
    assert cli.main(["flagstat", "-B", a, "-o", str(tmp_path / "a.txt"), "--hostDecode", "--anyOrder", "--threads", "2"]) == 0
    assert "not in coordinate order" not in capsys.readouterr().out
    assert open(str(tmp_path / "a.txt")).read() == open(str(tmp_path / "b.txt")).read()
