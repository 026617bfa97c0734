"""``--anyOrder`` on the GPU (``spl_bam_set_any_order``): the stable radix sort itself (csrc/spl_sort.hip through
``spl_sort_keys_device``) against numpy's stable argsort, the device decode of files whose records come in any order against the
host decoder and against numpy's stable sort of the records that were written (``ordercases``), and the commands end to end against
their own output for the sorted file and against the oracle.  Everything is exact.  The reference has no counterpart: it reads
through ``samtools view BAM region`` (SpliSER_v0_1_8.py:422), which needs ``samtools sort`` first."""
import numpy as np
import pytest

import ordercases as O
import xscases as X
from spliser_amd import cli, native, process as proc, readstore, synth
from test_gpu_configs import _oracle_tsv

pytestmark = pytest.mark.gpu
TILE = 1024        # (splsort::TILE: 16 rounds of 64 keys)
MAX_PARTS = 2048   # (splsort::MAX_PARTS: beyond this many tiles a wave walks several)


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


# ---- the sort itself ---------------------------------------------------------------------------------------------------------------

def _check_sort(ctx, name, keys, bits):
    got = native.sort_keys_device(ctx, keys, bits)
    assert np.array_equal(got, np.argsort(keys, kind="stable").astype(np.uint32)), name


def test_the_sort_at_its_edge_shapes(ctx):
    for name, keys, bits in O.sort_cases(TILE):
        _check_sort(ctx, name, keys, bits)
    n = 3 * TILE + 5
    assert np.array_equal(native.sort_keys_device(ctx, np.full(n, 0x0000000300001234, np.uint64), 40), np.arange(n, dtype=np.uint32))


def test_the_sort_over_many_tiles(ctx):
    """300 000 random keys of 40 bits -- 293 tiles, all five passes, a digit of the reference id in use -- and 300 000 keys drawn from
    seven values: runs of equal keys far longer than a tile, where only a stable pass leaves the permutation numpy's."""
    rng = np.random.default_rng(77)
    _check_sort(ctx, "random", rng.integers(0, 1 << 40, 300_000, dtype=np.uint64), 40)
    seven = rng.integers(0, 1 << 40, 7, dtype=np.uint64)
    _check_sort(ctx, "seven values", seven[rng.integers(0, 7, 300_000)], 40)


def test_the_sort_with_several_tiles_a_wave(ctx):
    """More tiles than waves in a launch: a wave walks two tiles, its digits' offsets running on in shared memory."""
    rng = np.random.default_rng(78)
    n = MAX_PARTS * TILE + 777
    _check_sort(ctx, "two tiles a wave", rng.integers(0, 1 << 26, n, dtype=np.uint64) | (rng.integers(0, 5, n, dtype=np.uint64) << np.uint64(32)), 35)


# ---- the device decode under the switch --------------------------------------------------------------------------------------------

def _device(path, ctx, **kw):
    bam = native.BamFile(path, threads=3, defer=True, **kw)
    bam.decode_on_device(ctx)
    return bam


def _host(path, **kw):
    bam = native.BamFile(path, threads=3, defer=True, **kw)
    bam.start_host_decode()
    return bam


def _check_file(ctx, path, names, mixed, read_filter=(0, 0, 0), aux_strand=False, sorts=True):
    """The device decode and the host decode of ``path`` under the switch hand out, per reference, numpy's stable sort of the
    records that were written; -> the device's BamFile (open)."""
    kw = dict(any_order=True, aux_strand=aux_strand, min_mapq=read_filter[0], require_flags=read_filter[1], exclude_flags=read_filter[2])
    dev, host = _device(path, ctx, **kw), _host(path, **kw)
    assert dev.on_device is True, dev.decline_reason()
    assert dev.wait_all() is True and host.wait_all() is True
    assert dev.decline_reason() == ""
    want = O.expected(mixed, len(names), read_filter)
    n_placed = sum(w.n for w, _ in want.values())
    assert dev.any_order_sorted() == ((n_placed, True) if sorts else (0, False))
    assert host.any_order_sorted() == ((n_placed, False) if sorts else (0, False))
    for tid, name in enumerate(names):
        d, h = dev.reads(name), host.reads(name)
        assert O.same_reads(d, want[tid][0]), name
        assert O.same_reads(h, want[tid][0]), name
        if want[tid][0].n:
            assert np.all(np.diff(d.pos.astype(np.int64)) >= 0)
            assert dev.wait_ref(name) == host.wait_ref(name)
            if aux_strand:
                xs = X.expected_xs(want[tid][0], want[tid][1])
                assert np.array_equal(d.xs, xs) and np.array_equal(h.xs, xs), name
    host.close()
    return dev


@pytest.fixture(scope="module")
def workload(tmp_path_factory):
    """``synth.Workload("arabidopsis", scale=0.005)``, five references: in coordinate order and shuffled by a seed, with its BED file."""
    d = tmp_path_factory.mktemp("anyorder")
    wl = synth.Workload("arabidopsis", scale=0.005, seed=6, workers=2)
    a, b, bed = str(d / "sorted.bam"), str(d / "shuffled.bam"), str(d / "x.bed")
    mixed = O.shuffle_workload(wl, a, b, seed=19)
    synth.write_bed(bed, wl.genome.chrom_names, wl.junctions)
    return wl, a, b, bed, mixed


def test_a_shuffled_workload_on_the_device(ctx, workload):
    wl, a, b, bed, mixed = workload
    names = wl.genome.chrom_names
    dev = _check_file(ctx, b, names, mixed)
    srt = _device(a, ctx)
    for tid, name in enumerate(names):
        assert O.multiset(dev.reads(name)) == O.multiset(srt.reads(name)) == O.multiset(wl.reads[tid])
    dev.close()
    srt.close()


def test_the_same_file_without_the_switch_goes_to_the_host(ctx, workload):
    wl, a, b, bed, mixed = workload
    off = _device(b, ctx)
    assert off.on_device is False and off.decline_reason() == "not sorted by reference"
    assert off.wait_all() is False
    off.close()


def test_a_sorted_file_under_the_switch_is_left_as_it_is(ctx, workload):
    wl, a, b, bed, mixed = workload
    on, off = _device(a, ctx, any_order=True), _device(a, ctx)
    assert on.on_device is True and off.on_device is True
    assert on.wait_all() is True and on.any_order_sorted() == (0, False)
    for name in wl.genome.chrom_names:
        x, y = on.reads(name), off.reads(name)
        for f in ("pos", "flag", "cig_off", "cigar"):
            assert getattr(x, f).tobytes() == getattr(y, f).tobytes(), (name, f)
    on.close()
    off.close()


def test_strand_bytes_travel_with_their_reads(ctx, tmp_path):
    """XS-tagged spliced reads (the records of xscases, written through ordercases), shuffled: the fifth array in the new order."""
    rng = np.random.default_rng(8)
    sets, tags = [], []
    for _ in range(3):
        rs = X.make_reads(rng, 1500)
        t, _ = X.make_tags(rng, rs)
        sets.append(rs)
        tags.append(t)
    mixed = O.shuffled(O.records_of(sets, tags=tags), 5)
    path = str(tmp_path / "xs.bam")
    O.write_bam(path, ["a", "b", "c"], [10 ** 6] * 3, mixed)
    _check_file(ctx, path, ["a", "b", "c"], mixed, aux_strand=True).close()
    _check_file(ctx, path, ["a", "b", "c"], mixed, read_filter=(0, 0, 0x100), aux_strand=True).close()


M = lambda n: (n << 4)          # noqa: E731
N = lambda n: (n << 4) | 3      # noqa: E731


def test_hand_built_files(ctx, tmp_path):
    spliced = [M(20), N(300), M(30)]
    cases = {
        "one record per reference in descending tid": (["r%d" % t for t in range(40)], [(t, 100 + t, 0, 60, [M(50)], b"") for t in range(39, -1, -1)]),
        "300 references, one read on each": (["r%d" % t for t in range(300)], O.shuffled([(t, 1 + (t * 7919) % 1000, 16 * (t & 1), 60, [M(10 + t % 7)], b"") for t in range(300)], 3)),
        "no CIGAR and unmapped-but-placed reads among spliced ones": (
            ["a", "b"],
            O.shuffled([(k & 1, 1 + (k * 37) % 500, 4 if k % 5 == 0 else 0, 60, [] if k % 3 == 0 else (spliced if k % 3 == 1 else [M(75)]), b"") for k in range(60)]
                       + [(-1, 0, 4, 0, [], b"")] * 3, 4)),
        "a reference with no reads": (["a", "none", "b", "none2"], O.shuffled([(2 * (k % 2), 10 + k % 17, 0, 60, spliced if k % 4 == 0 else [M(40)], b"") for k in range(50)], 5)),
        "equal coordinates keep the file's order": (["a", "b"], [(k % 2, 7, k, 60, [M(1 + k)], b"") for k in range(48)][::-1] + [(0, 7, 99, 60, [M(5)], b""), (0, 3, 98, 60, [], b"")]),
    }
    for title, (names, recs) in cases.items():
        path = str(tmp_path / "h.bam")
        O.write_bam(path, names, [10 ** 6] * len(names), recs)
        _check_file(ctx, path, names, recs).close()
    # POS of 2^31 - 2 (0-based: 2^31 - 1 as the arrays keep it) on a header that allows it: all 31 bits of the key's low word
    top = (1 << 31) - 1
    recs = [(1, top, 0, 60, [M(1)], b""), (0, 5, 0, 60, [M(10)], b""), (1, 1 << 30, 16, 60, [M(3)], b""), (0, top, 0, 60, [], b""), (1, 9, 0, 60, spliced, b"")]
    path = str(tmp_path / "top.bam")
    O.write_bam(path, ["a", "b"], [top, top], recs)
    dev = _check_file(ctx, path, ["a", "b"], recs)
    assert dev.reads("b").pos.tolist() == [9, 1 << 30, top]
    dev.close()


@pytest.mark.parametrize("window", ["2", "5"])
def test_a_decode_of_several_windows(ctx, workload, monkeypatch, window):
    """Windows of a few blocks (SPL_INFLATE_WINDOW_BLOCKS, as tests/test_gpu_bam_device.py gets them): the records of a shuffled
    file extracted window by window, the arrays growing as they go, sorted behind the last one."""
    wl, a, b, bed, mixed = workload
    monkeypatch.setenv("SPL_INFLATE_WINDOW_BLOCKS", window)
    _check_file(ctx, b, wl.genome.chrom_names, mixed).close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

def _run(argv, capsys):
    capsys.readouterr()
    assert cli.main(argv) == 0
    proc.wait_deferred_close()
    return capsys.readouterr().out


def test_process_with_a_junction_file(workload, tmp_path, capsys, oracle_lib):
    wl, a, b, bed, mixed = workload
    for tag, extra, stranded, cryptic in (("u", [], None, False), ("s", ["--isStranded", "-s", "fr", "--beta2Cryptic"], "fr", True)):
        o1, o2 = str(tmp_path / (tag + "1")), str(tmp_path / (tag + "2"))
        out = _run(["process", "-B", b, "-b", bed, "-o", o1, "--anyOrder"] + extra, capsys)
        assert "the alignment file is not in coordinate order: %d reads sorted on the GPU" % sum(rs.n for rs in wl.reads) in out
        assert "counting again" not in out and "decoded on host threads" not in out
        _run(["process", "-B", a, "-b", bed, "-o", o2] + extra, capsys)
        got = open(o1 + ".SpliSER.tsv").read()
        assert got == open(o2 + ".SpliSER.tsv").read()
        assert got == _oracle_tsv(oracle_lib, bed, wl, stranded, cryptic)


def test_process_without_a_junction_file_and_junctions(workload, tmp_path, capsys):
    wl, a, b, bed, mixed = workload
    o1, o2 = str(tmp_path / "n1"), str(tmp_path / "n2")
    _run(["process", "-B", b, "-o", o1, "--anyOrder", "--keepJunctions"], capsys)
    _run(["process", "-B", a, "-o", o2, "--keepJunctions"], capsys)
    assert open(o1 + ".SpliSER.tsv").read() == open(o2 + ".SpliSER.tsv").read()
    assert open(o1 + ".junctions.bed").read() == open(o2 + ".junctions.bed").read()
    assert len(open(o1 + ".SpliSER.tsv").read().splitlines()) > 50
    _run(["junctions", "-B", b, "-o", o1 + ".bed", "--anyOrder"], capsys)
    _run(["junctions", "-B", a, "-o", o2 + ".bed"], capsys)
    assert open(o1 + ".bed").read() == open(o2 + ".bed").read() == open(o2 + ".junctions.bed").read()


def test_flagstat_filter_and_kept_reads(workload, tmp_path, capsys):
    wl, a, b, bed, mixed = workload
    o1, o2 = str(tmp_path / "f1"), str(tmp_path / "f2")
    _run(["process", "-B", b, "-b", bed, "-o", o1, "--anyOrder", "--flagstat", "--keepReads"], capsys)
    _run(["process", "-B", a, "-b", bed, "-o", o2, "--flagstat", "--keepReads"], capsys)
    assert open(o1 + ".flagstat.txt").read() == open(o2 + ".flagstat.txt").read()
    _run(["flagstat", "-B", b, "-o", o1 + ".txt", "--anyOrder"], capsys)
    assert open(o1 + ".txt").read() == open(o2 + ".flagstat.txt").read()
    # the kept reads are the sorted reads: per reference numpy's stable sort of what was written, the sorted file's as a multiset
    k1, k2 = readstore.open_if_fresh(o1 + readstore.SUFFIX, b), readstore.open_if_fresh(o2 + readstore.SUFFIX, a)
    want = O.expected(mixed, 5)
    for tid, name in enumerate(wl.genome.chrom_names):
        assert O.same_reads(k1.reads(name), want[tid][0]), name
        assert O.multiset(k1.reads(name)) == O.multiset(k2.reads(name))
    # a read filter (the files' MAPQ is drawn from 0..60: one read in six goes)
    argv = ["--minMapQ", "10", "--excludeFlags", "0x900"]
    _run(["process", "-B", b, "-b", bed, "-o", o1 + "q", "--anyOrder"] + argv, capsys)
    _run(["process", "-B", a, "-b", bed, "-o", o2 + "q"] + argv, capsys)
    assert open(o1 + "q.SpliSER.tsv").read() == open(o2 + "q.SpliSER.tsv").read()
    assert open(o1 + "q.SpliSER.tsv").read() != open(o1 + ".SpliSER.tsv").read()


def test_nothing_changes_without_the_flag(workload, tmp_path, capsys, oracle_lib):
    wl, a, b, bed, mixed = workload
    o = str(tmp_path / "p")
    out = _run(["process", "-B", b, "-b", bed, "-o", o], capsys)
    assert "counting again from the complete decode" in out and "sorted on the GPU" not in out
    assert open(o + ".SpliSER.tsv").read() == _oracle_tsv(oracle_lib, bed, wl, None, False)
    with pytest.raises(native.SpliserNativeError, match="sort it"):
        cli.main(["junctions", "-B", b, "-o", o + ".bed"])
    with pytest.raises(native.SpliserNativeError, match="sort it"):
        cli.main(["process", "-B", b, "-o", o + "n"])
    proc.wait_deferred_close()


def test_a_sorted_file_with_the_flag(workload, tmp_path, capsys):
    wl, a, b, bed, mixed = workload
    o1, o2 = str(tmp_path / "s1"), str(tmp_path / "s2")
    out = _run(["process", "-B", a, "-o", o1, "--anyOrder", "--keepJunctions", "--keepReads"], capsys)
    assert "not in coordinate order" not in out
    _run(["process", "-B", a, "-o", o2, "--keepJunctions", "--keepReads"], capsys)
    for suffix in (".SpliSER.tsv", ".junctions.bed"):
        assert open(o1 + suffix).read() == open(o2 + suffix).read()
    assert open(o1 + readstore.SUFFIX, "rb").read() == open(o2 + readstore.SUFFIX, "rb").read()
    out = _run(["process", "-B", a, "-b", bed, "-o", o1 + "b", "--anyOrder"], capsys)
    assert "not in coordinate order" not in out
    _run(["process", "-B", a, "-b", bed, "-o", o2 + "b"], capsys)
    assert open(o1 + "b.SpliSER.tsv").read() == open(o2 + "b.SpliSER.tsv").read()


def test_several_devices_decode_the_file_whole(workload, tmp_path, capsys, oracle_lib):
    wl, a, b, bed, mixed = workload
    o = str(tmp_path / "m")
    out = _run(["process", "-B", b, "-b", bed, "-o", o, "--anyOrder", "--devices", "0,0,0"], capsys)
    assert "decoded whole on device 0, not in shares over 3 devices" in out and "sorted on the GPU" in out
    assert open(o + ".SpliSER.tsv").read() == _oracle_tsv(oracle_lib, bed, wl, None, False)
