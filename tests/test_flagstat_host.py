"""The flagstat counters (``spl_bam_set_flagstat``) without a GPU: the one definition (csrc/spl_flagstat.h, through
``spl_flagstat_add_host``) against the restatement of its table for every flag value, the host decoder on hand-built files --
whole, under read filters, with one thread and four --, the rules of the switch, and the text the commands write."""
import os

import numpy as np
import pytest

import filtercases as F
import flagstatcases as fc
from spliser_amd import cli, flagstat, native

MAPQS = (0, 4, 5, 255)
MATES = ((2, 2), (2, 3), (2, -1))      # (tid, next_tid): same chromosome, a different one, no mate chromosome


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


@pytest.fixture(scope="module")
def mixed():
    return fc.mix(seed=3, n=500, body=90)


def _file(tmp_path, b, lens, name="f.bam"):
    return b.write(str(tmp_path / name), lens)


def test_the_definition_for_every_flag_value(built):
    """4096 flag values x three mate placements x four MAPQs, one record at a time: the C function adds exactly what the table says."""
    flags = np.arange(4096)
    for tid, next_tid in MATES:
        for mapq in MAPQS:
            got = np.zeros((4096, 16, 2), np.int64)
            for f in flags:
                native.flagstat_add_host(int(f), tid, next_tid, mapq, got[f])
            rows, failed = fc.masks(flags, np.full(4096, tid), np.full(4096, next_tid), np.full(4096, mapq))
            want = np.zeros((4096, 16, 2), np.int64)
            want[:, :, 0] = (rows & ~failed).T
            want[:, :, 1] = (rows & failed).T
            bad = np.flatnonzero((got != want).any(axis=(1, 2)))
            assert len(bad) == 0, (hex(int(bad[0])), tid, next_tid, mapq, got[bad[0]].T, want[bad[0]].T)
    # ... and accumulated: all of them into one set of counters
    acc = np.zeros((16, 2), np.int64)
    for f in range(0, 4096, 7):
        native.flagstat_add_host(f, 0, 1, 5, acc)
    fl = np.arange(0, 4096, 7)
    assert np.array_equal(acc, fc.restate(fl, np.zeros_like(fl), np.ones_like(fl), np.full_like(fl, 5)))


def test_bits_above_the_twelve_change_nothing(built):
    for f in (0x1 | 0x40, 0x900, 0x4):
        assert np.array_equal(native.flagstat_add_host(f | 0xF000, 1, 0, 9), native.flagstat_add_host(f, 1, 0, 9))


@pytest.mark.parametrize("threads", [1, 4])
def test_host_decoder_counts_every_record(built, mixed, tmp_path, threads, monkeypatch):
    monkeypatch.setenv("SPL_BAM_BATCH_BLOCKS", "3")        # (many batches: records straddle them, their counters are added in order)
    for k, L in enumerate((700, 4096, 65536)):
        path = _file(tmp_path, mixed, mixed.tiles(L), "m%d.bam" % k)
        bam = native.BamFile(path, threads=threads, flagstat=True)
        got = bam.flagstat()
        assert np.array_equal(got, mixed.want()), (L, got.T, mixed.want().T)
        assert got[0].sum() == bam.n_records == mixed.n_records
        bam.close()


def test_host_decoder_resync_counts_once(built, mixed, tmp_path, monkeypatch):
    """Every batch walked again from the known boundary (the path a wrong guess takes): the worker's own counters are dropped with its parts."""
    monkeypatch.setenv("SPL_BAM_BATCH_BLOCKS", "2")
    monkeypatch.setenv("SPL_BAM_FORCE_RESYNC", "1")
    bam = native.BamFile(_file(tmp_path, mixed, mixed.tiles(1500)), threads=4, flagstat=True)
    assert np.array_equal(bam.flagstat(), mixed.want())
    bam.close()


@pytest.mark.parametrize("filt", [F.FILTER_A, F.FILTER_B, (5, 0, 0)])
@pytest.mark.parametrize("threads", [1, 4])
def test_under_a_filter_the_counters_are_the_prefiltered_files(built, mixed, tmp_path, filt, threads):
    path = _file(tmp_path, mixed, mixed.tiles(2000))
    plain = native.BamFile(path, threads=threads, min_mapq=filt[0], require_flags=filt[1], exclude_flags=filt[2])
    bam = native.BamFile(path, threads=threads, min_mapq=filt[0], require_flags=filt[1], exclude_flags=filt[2], flagstat=True)
    got, want = bam.flagstat(), mixed.want(filt)
    assert np.array_equal(got, want), (got.T, want.T)
    assert not np.array_equal(want, mixed.want())
    # unmapped records without a reference fail --minMapQ too: they are in the unfiltered counters and not in these
    unplaced = mixed.tid < 0
    keep = F.keep_mask(mixed.flag, mixed.mapq, filt)[0]
    assert (unplaced & ~keep).sum() > 0
    assert got[0].sum() == int(keep.sum())
    # n_records and filter_counts keep their meaning (placeable records only) and their values
    assert bam.n_records == plain.n_records == mixed.n_records
    assert bam.filter_counts() == plain.filter_counts()
    placeable = mixed.tid >= 0
    _, by_flags, by_mapq = F.keep_mask(mixed.flag[placeable], mixed.mapq[placeable], filt)
    assert bam.filter_counts() == (int(by_flags.sum()), int(by_mapq.sum()))
    bam.close()
    plain.close()


def test_the_switch(built, mixed, tmp_path):
    path = _file(tmp_path, mixed, mixed.tiles(3000))
    off = native.BamFile(path, threads=2)
    with pytest.raises(native.SpliserNativeError) as e:
        off.flagstat()
    assert e.value.code == -1 and "switched on" in str(e.value)
    with pytest.raises(native.SpliserNativeError) as e:      # (decoded already)
        off.set_flagstat(True)
    assert e.value.code == -1
    late = native.BamFile(path, threads=2, defer=True)
    late.start_host_decode()
    with pytest.raises(native.SpliserNativeError) as e:
        late.set_flagstat(True)
    assert e.value.code == -1
    # off and on: the same reads, the same counters of the filter
    on = native.BamFile(path, threads=2, flagstat=True)
    for t in range(mixed.n_ref):
        a, b = off.reads("c%d" % t), on.reads("c%d" % t)
        F.same_reads(a, b, "c%d" % t)
    assert off.filter_counts() == on.filter_counts() == (0, 0) and off.n_records == on.n_records
    # switched on and off again before the decode: off
    back = native.BamFile(path, threads=2, defer=True)
    back.set_flagstat(True)
    back.set_flagstat(False)
    with pytest.raises(native.SpliserNativeError):
        back.flagstat()
    for b in (off, late, on, back):
        b.close()


HAND = """7 + 2 in total (QC-passed reads + QC-failed reads)
6 + 1 primary
1 + 0 secondary
0 + 1 supplementary
2 + 0 duplicates
1 + 0 primary duplicates
5 + 2 mapped (71.43% : 100.00%)
4 + 1 primary mapped (66.67% : 100.00%)
0 + 0 paired in sequencing
0 + 0 read1
0 + 0 read2
0 + 0 properly paired (N/A : N/A)
0 + 0 with itself and mate mapped
0 + 0 singletons (N/A : N/A)
0 + 0 with mate mapped to a different chr
0 + 0 with mate mapped to a different chr (mapQ>=5)
"""

HAND_PAIRED = """3 + 0 in total (QC-passed reads + QC-failed reads)
3 + 0 primary
0 + 0 secondary
0 + 0 supplementary
0 + 0 duplicates
0 + 0 primary duplicates
3 + 0 mapped (100.00% : N/A)
3 + 0 primary mapped (100.00% : N/A)
3 + 0 paired in sequencing
2 + 0 read1
1 + 0 read2
1 + 0 properly paired (33.33% : N/A)
2 + 0 with itself and mate mapped
1 + 0 singletons (33.33% : N/A)
1 + 0 with mate mapped to a different chr
1 + 0 with mate mapped to a different chr (mapQ>=5)
"""


def _hand(tmp_path):
    """Nine single-end records: four primary mapped, two primary unmapped, a secondary duplicate, a primary duplicate among the
    mapped, and two that failed quality control (one of them supplementary)."""
    rows = [(0x0, 0), (0x10, 0), (0x0, 0), (0x400, 0), (0x100 | 0x400, 0), (0x200, 1), (0x200 | 0x800, 1), (0x4, -1), (0x4, -1)]
    recs = [fc._rec(t, 10 + k if t >= 0 else -1, f, 60, -1) for k, (f, t) in enumerate(rows)]
    b = fc.Built(2, recs, [(f, t, -1, 60) for f, t in rows])
    rows2 = [(0x1 | 0x2 | 0x40, 0, 0), (0x1 | 0x80, 0, 1), (0x1 | 0x8 | 0x40, 1, 1)]
    recs2 = [fc._rec(t, 10 + k, f, 60, nt) for k, (f, t, nt) in enumerate(rows2)]
    b2 = fc.Built(2, recs2, [(f, t, nt, 60) for f, t, nt in rows2])
    return b.write(str(tmp_path / "hand.bam"), [len(b.stream)]), b2.write(str(tmp_path / "hand2.bam"), [len(b2.stream)])


def test_the_text_by_hand(built, tmp_path, capsys):
    single, paired = _hand(tmp_path)
    out = str(tmp_path / "hand.txt")
    assert cli.main(["flagstat", "-B", single, "-o", out, "--hostDecode"]) == 0
    assert open(out).read() == HAND
    assert "Library size: 5 mapped reads (4 primary)" in capsys.readouterr().out
    assert cli.main(["flagstat", "-B", paired, "-o", out, "--hostDecode", "--threads", "1"]) == 0
    assert open(out).read() == HAND_PAIRED


def test_flagstat_command_on_host_threads(built, tmp_path, capsys):
    """(``process --flagstat --hostDecode`` counts on the GPU and is in test_gpu_flagstat.py.)"""
    c = F.Case("junctions_u", 11, F.FILTER_A)
    x, kept = c.write(str(tmp_path / "p"), with_seq=True)
    flag = np.concatenate([rs.flag for _, rs in c.x])
    mapq = np.concatenate(c.mapq)
    tid = np.concatenate([np.full(rs.n, k) for k, (_, rs) in enumerate(c.x)])
    none = np.full(len(flag), -1)
    out = lambda tag: str(tmp_path / tag)      # noqa: E731
    for tag, filt, argv in (("all", (0, 0, 0), []), ("a", F.FILTER_A, ["--minMapQ", "255", "--excludeFlags", "0x900"])):
        w = fc.restate_filtered(flag, tid, none, mapq, filt)
        want = "\n".join(flagstat.format_lines(w)) + "\n"
        capsys.readouterr()
        assert cli.main(["flagstat", "-B", x, "-o", out(tag + ".txt"), "--hostDecode", "--threads", "3"] + argv) == 0
        assert open(out(tag + ".txt")).read() == want
        assert "Library size: %d mapped reads (%d primary)" % (w[6, 0], w[7, 0]) in capsys.readouterr().out
    assert open(out("a.txt")).read() != open(out("all.txt")).read()
    # the pre-filtered file without the flags: the same text
    assert cli.main(["flagstat", "-B", kept, "-o", out("kept.txt"), "--hostDecode"]) == 0
    assert open(out("kept.txt")).read() == open(out("a.txt")).read()


def test_sam_text_has_no_counters(built, tmp_path):
    c = F.Case("junctions_u", 11, F.FILTER_A)
    with pytest.raises(native.SpliserNativeError):
        flagstat.flagstat(os.path.join(c.dir, "reads.sam"), str(tmp_path / "x.txt"), gpuDecode=False)
