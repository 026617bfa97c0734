"""Read filters (--minMapQ / --requireFlags / --excludeFlags; ``spl_bam_set_filter``) without a GPU: the host decoder under a filter
gives what it gives for the file filtered beforehand (``filtercases``: X and X'), the counts are numpy's, the SAM reader follows
the same rule, the command line refuses what cannot be meant, kept reads know the filter they were kept under, and the one
predicate of ``spl_bam.h`` -- compiled with plain g++ -- is samtools' rule over every MAPQ."""
import ctypes
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import filtercases as F
from spliser_amd import cli, native, process as proc, readstore, samio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("junctions_u", 11, F.FILTER_A, None), ("random_a", 12, F.FILTER_B, "fr"), ("random_b", 13, F.FILTER_A, None)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    native.build()


@pytest.mark.parametrize("case,seed,filt,stranded", CASES)
def test_the_cases_are_cases(case, seed, filt, stranded, oracle_lib):
    """What every test below and on the GPU relies on: reads dropped either way, a spliced read kept (``Case`` asserts those),
    and an oracle whose beta1 is not the same for X and X'."""
    F.Case(case, seed, filt).assert_beta1_differs(oracle_lib, stranded)


def _check_file(path_x, path_kept, c, threads, unplaced=0):
    want = native.BamFile(path_kept, threads=threads)
    got = native.BamFile(path_x, threads=threads, min_mapq=c.filt[0], require_flags=c.filt[1], exclude_flags=c.filt[2])
    try:
        for (chrom, sub) in c.x_kept:
            F.same_reads(got.reads(chrom), sub, chrom)
            w = want.reads(chrom)
            F.same_reads(got.reads(chrom), w if w is not None and w.n else samio.ReadSet.empty(), chrom)
            assert got.wait_ref(chrom) == want.wait_ref(chrom)
        assert got.filter_counts() == (c.by_flags, c.by_mapq)
        assert want.filter_counts() == (0, 0)
        assert got.n_records == c.n_all + unplaced and want.n_records == c.n_kept + unplaced
    finally:
        got.close()
        want.close()


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("case,seed,filt,stranded", CASES)
def test_host_decoder_under_a_filter_gives_the_prefiltered_file(case, seed, filt, stranded, threads, tmp_path, monkeypatch):
    c = F.Case(case, seed, filt)
    for tag, kw in (("plain", {}), ("cg", dict(long_cigar_tag=True)), ("unplaced", dict(unplaced=7, with_seq=True))):
        x, kept = c.write(str(tmp_path / tag), **kw)
        _check_file(x, kept, c, threads, kw.get("unplaced", 0))
    monkeypatch.setenv("SPL_BAM_BATCH_BLOCKS", "1")       # (batches of one block: records straddle them, the committing thread bridges)
    monkeypatch.setenv("SPL_BAM_FORCE_RESYNC", "1")       # (... and every batch walked again sequentially)
    _check_file(x, kept, c, threads, 7)


def test_defaults_keep_every_record(tmp_path):
    c = F.Case("junctions_u", 11, F.FILTER_A)
    x, _ = c.write(str(tmp_path / "d"))
    for kw in ({}, dict(min_mapq=0, require_flags=0, exclude_flags=0)):
        bam = native.BamFile(x, threads=2, **kw)
        for chrom, full in c.x:
            F.same_reads(bam.reads(chrom), full, chrom)
        assert bam.filter_counts() == (0, 0) and bam.n_records == c.n_all
        bam.close()


def test_mapq_255_passes_any_threshold(tmp_path):
    rs = samio.ReadSet.from_records([(0, 10, "50M"), (0, 20, "20M100N30M"), (0, 30, "50M")])
    path = str(tmp_path / "q.bam")
    samio.write_bam(path, ["c"], [10 ** 6], [("c", rs)], mapq=[np.array([255, 254, 0])])
    bam = native.BamFile(path, threads=1, min_mapq=255)
    assert bam.reads("c").pos.tolist() == [10] and bam.filter_counts() == (0, 2)
    bam.close()


def test_set_filter_is_refused_once_a_decode_has_started(tmp_path):
    c = F.Case("junctions_u", 11, F.FILTER_A)
    x, _ = c.write(str(tmp_path / "s"))
    bam = native.BamFile(x, threads=2, defer=True)
    bam.set_filter(*F.FILTER_A)
    bam.set_filter(*F.FILTER_B)        # (still nobody's: may be changed)
    for bad in ((256, 0, 0), (-1, 0, 0), (0, 65536, 0), (0, 0, -2)):
        with pytest.raises(native.SpliserNativeError):
            bam.set_filter(*bad)
    bam.start_host_decode()
    with pytest.raises(native.SpliserNativeError, match="decoded"):
        bam.set_filter(*F.FILTER_A)
    bam.wait_all()
    with pytest.raises(native.SpliserNativeError):
        bam.set_filter(0, 0, 0)
    masks = [F.keep_mask(rs.flag, m, F.FILTER_B) for (_, rs), m in zip(c.x, c.mapq)]      # (the filter set last is the one that holds)
    assert bam.filter_counts() == (sum(int(m[1].sum()) for m in masks), sum(int(m[2].sum()) for m in masks))
    bam.close()
    for kw in (dict(stream=True), {}):   # (files whose decode the opening call starts)
        bam = native.BamFile(x, threads=2, **kw)
        with pytest.raises(native.SpliserNativeError):
            bam.set_filter(*F.FILTER_A)
        bam.close()
    bam = native.BamFile(x, threads=2, defer=True)
    bam.wait_ref(c.names[0])           # (a wait starts the host decode)
    with pytest.raises(native.SpliserNativeError):
        bam.set_filter(*F.FILTER_A)
    bam.close()


def test_share_counts_on_the_host_leave_the_dropped_records_out(tmp_path):
    c = F.Case("junctions_u", 11, F.FILTER_A, repeat=4)
    x, _ = c.write(str(tmp_path / "h"), with_seq=True, unplaced=3)
    bam = native.BamFile(x, threads=2, defer=True, min_mapq=c.filt[0], require_flags=c.filt[1], exclude_flags=c.filt[2])
    n = ctypes.c_int(0)
    native._check(native.lib().spl_bam_share_plan(bam._h, ctypes.c_int(3), ctypes.byref(n)))
    assert n.value == 3
    total = np.sum([bam.share_count_host(k) for k in range(n.value)], axis=0)
    assert total.tolist() == [rs.n for _, rs in c.x_kept] + [3]
    bam.close()


@pytest.mark.parametrize("case,seed,filt,stranded", CASES)
def test_sam_text_follows_the_same_rule(case, seed, filt, stranded, tmp_path):
    c = F.Case(case, seed, filt)
    path = str(tmp_path / "x.sam")
    samio.write_sam(path, c.names, c.lengths, c.x, mapq=c.mapq)
    src = proc.open_alignments(path, options=proc.DecodeOptions(read_filter=c.filt))
    for chrom, sub in c.x_kept:
        F.same_reads(src.reads(chrom), sub, chrom)
    assert src.filter_counts() == (c.by_flags, c.by_mapq) and src.n_records == c.n_all
    names, sets = samio.read_sam(path)
    for chrom, full in c.x:
        F.same_reads(sets[chrom], full, chrom)
    plain = str(tmp_path / "plain.sam")       # (the writers' default MAPQ is the 60 it always was)
    samio.write_sam(plain, c.names, c.lengths, c.x)
    assert {line.split("\t")[4] for line in open(plain) if not line.startswith("@")} == {"60"}


@pytest.mark.parametrize("argv,message", [
    (["--minMapQ", "256"], "--minMapQ must be in 0..255"),
    (["--minMapQ", "-1"], "--minMapQ must be in 0..255"),
    (["--requireFlags", "65536"], "must be in 0..65535"),
    (["--excludeFlags", "-1"], "must be in 0..65535"),
    (["--excludeFlags", "0x10000"], "must be in 0..65535"),
    (["--requireFlags", "0x3", "--excludeFlags", "0x902"], "share a bit"),
    (["--excludeFlags", "abc"], "invalid"),
])
@pytest.mark.parametrize("command", ["process", "junctions", "combine", "combineShallow"])
def test_the_command_line_refuses_what_cannot_be_meant(command, argv, message, capsys):
    base = {"process": ["process", "-B", "x.bam", "-o", "out"], "junctions": ["junctions", "-B", "x.bam", "-o", "out.bed"],
            "combine": ["combine", "-S", "samples.tsv", "-o", "out"], "combineShallow": ["combineShallow", "-S", "samples.tsv", "-o", "out"]}[command]
    with pytest.raises(SystemExit) as exc:
        cli.main(base + argv)
    assert exc.value.code == 2
    assert message in capsys.readouterr().err


def test_flag_masks_are_read_like_samtools_reads_them():
    args = cli.build_parser().parse_args(["process", "-B", "x", "-o", "y", "--excludeFlags", "0x900", "--requireFlags", "0b11", "--minMapQ", "255"])
    assert (args.minMapQ, args.requireFlags, args.excludeFlags) == (255, 3, 2304)
    args = cli.build_parser().parse_args(["junctions", "-B", "x", "-o", "y", "--excludeFlags", "2304"])
    assert (args.minMapQ, args.requireFlags, args.excludeFlags) == (0, 0, 2304)
    assert proc.read_filter(255, 0, 0x900) == (255, 0, 0x900) and proc.read_filter() == proc.NO_FILTER
    for bad in ((256, 0, 0), (0, 1 << 16, 0), (0, 4, 4)):
        with pytest.raises(ValueError):
            proc.read_filter(*bad)


def _head(path):
    with open(path, "rb") as fh:
        fixed = fh.read(16)
        version, n = struct.unpack("<II", fixed[8:16])
        raw = fh.read(n)
    return version, raw, json.loads(raw.decode("utf-8"))


def test_kept_reads_know_their_filter(tmp_path):
    c = F.Case("junctions_u", 11, F.FILTER_A)
    x, _ = c.write(str(tmp_path / "k"))
    a, b, none = str(tmp_path / "a.SpliSER.reads"), str(tmp_path / "b.SpliSER.reads"), str(tmp_path / "n.SpliSER.reads")
    readstore.save(a, x, c.x_kept, read_filter=F.FILTER_A)
    assert readstore.open_if_fresh(a, x) is None
    assert readstore.open_if_fresh(a, x, F.FILTER_B) is None
    assert readstore.open_if_fresh(a, x, (255, 0, 0x800)) is None
    store = readstore.open_if_fresh(a, x, F.FILTER_A)
    assert store is not None
    for chrom, sub in c.x_kept:
        F.same_reads(store.reads(chrom), sub, chrom)
    store.close()
    assert _head(a)[2]["filter"] == {"min_mapq": 255, "require_flags": 0, "exclude_flags": 0x900}
    # an unfiltered save: no such key, and byte for byte the file of format version 2 -- the header is json.dumps of exactly these
    # keys in this order, the payload the arrays at 64-byte boundaries
    readstore.save(none, x, c.x)
    readstore.save(b, x, c.x, read_filter=(0, 0, 0))
    assert open(none, "rb").read() == open(b, "rb").read()
    version, raw, head = _head(none)
    assert version == 2 and list(head) == ["version", "bam_size", "bam_mtime_ns", "bam_crc32", "payload_sum", "refs"]
    assert json.dumps(head).encode("utf-8") == raw
    assert readstore.open_if_fresh(none, x) is not None and readstore.open_if_fresh(none, x, (0, 0, 0)) is not None
    assert readstore.open_if_fresh(none, x, F.FILTER_A) is None


def test_the_predicate_compiles_with_gcc_and_is_samtools_rule(tmp_path):
    """spl_bam.h's spl_bam_filter_verdict -- the one definition the host decoder and the kernels call -- built with plain g++ and
    held against numpy over all 256 MAPQ values x thresholds x flag / require / exclude triples."""
    src = str(tmp_path / "verdict.cpp")
    with open(src, "w") as fh:
        fh.write('#include "spl_bam.h"\n'
                 'extern "C" void verdicts(unsigned min_mapq, unsigned req, unsigned exc, const unsigned *flag, const unsigned *mapq, int n, int *out)\n'
                 '{ const spl_bam_filter f = {min_mapq, req, exc}; for (int i = 0; i < n; ++i) out[i] = spl_bam_filter_verdict(f, flag[i], mapq[i]); }\n')
    lib = str(tmp_path / "libverdict.so")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "spliser_amd", "csrc"), src, "-o", lib])
    fn = ctypes.CDLL(lib).verdicts
    flags = np.array([0, 1, 4, 16, 99, 147, 83, 163, 256, 272, 1024, 1040, 2048, 2064, 0x900, 0xF00, 0x200, 0xFFFF, 0x903, 355], np.uint32)
    masks = [0, 1, 2, 3, 4, 0x100, 0x400, 0x800, 0x900, 0xF00, 0x200, 0xFFFF, 0x10, 0x63]
    mapq_all = np.arange(256, dtype=np.uint32)
    flag = np.repeat(flags, 256)
    mapq = np.tile(mapq_all, len(flags))
    out = np.empty(flag.shape[0], np.int32)
    n_checked = 0
    for q in (0, 1, 2, 3, 4, 10, 30, 60, 61, 254, 255):
        for req in masks:
            for exc in masks:
                fn(ctypes.c_uint(q), ctypes.c_uint(req), ctypes.c_uint(exc), flag.ctypes.data_as(ctypes.c_void_p), mapq.ctypes.data_as(ctypes.c_void_p),
                   ctypes.c_int(flag.shape[0]), out.ctypes.data_as(ctypes.c_void_p))
                kept, by_flags, by_mapq = F.keep_mask(flag, mapq, (q, req, exc))
                assert np.array_equal(out, np.where(by_flags, 1, np.where(by_mapq, 2, 0))), (q, req, exc)
                n_checked += flag.shape[0]
    assert n_checked == 11 * len(masks) ** 2 * len(flags) * 256
