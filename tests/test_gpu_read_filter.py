"""Read filters (--minMapQ / --requireFlags / --excludeFlags; ``spl_bam_set_filter``) on the GPU: the device decode of X under a
filter leaves what the device decode of X' leaves (``filtercases``: X' = X without the reads the filter drops, taken out in
numpy) -- with the wave extraction and the walking one, with windows of a few blocks, in shares --, and the commands give for X
with the flags what they give for X' without them, which is what the oracle gives for X'.  The oracle never sees a filter."""
import os
import types

import pytest

import filtercases as F
from spliser_amd import cli, native, samio
from test_gpu_configs import _oracle_tsv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


def _flags(filt):
    return ["--minMapQ", str(filt[0]), "--requireFlags", hex(filt[1]), "--excludeFlags", hex(filt[2])]


def _kw(filt):
    return dict(min_mapq=filt[0], require_flags=filt[1], exclude_flags=filt[2])


def _decode(path, ctx, filt, devices=None):
    bam = native.BamFile(path, threads=2, defer=True, **_kw(filt))
    if devices is None:
        assert bam.decode_on_device(ctx) is True, bam.decline_reason()
    else:
        plan = bam.decode_on_devices_async(list(devices))
        assert len(plan) == len(devices)
        assert bam.join_decoders() is True, bam.decline_reason()
    return bam


def _same_files(c, x, kept, ctx, devices=None):
    """Device decode of X under the case's filter against device decode of X': arrays, per-reference counts, the counters."""
    got, want = _decode(x, ctx, c.filt, devices), _decode(kept, ctx, (0, 0, 0), devices)
    try:
        for chrom, sub in c.x_kept:
            assert got.wait_ref(chrom) == want.wait_ref(chrom), chrom
            assert got.wait_ref(chrom)[0] == sub.n
            F.same_reads(got.reads(chrom), sub, chrom)
            w = want.reads(chrom)
            F.same_reads(got.reads(chrom), w if w is not None and w.n else samio.ReadSet.empty(), chrom)
        assert got.filter_counts() == (c.by_flags, c.by_mapq) and want.filter_counts() == (0, 0)
        assert got.n_records == c.n_all and want.n_records == c.n_kept
        if devices is not None:
            cut = [chrom for chrom, _ in c.x if sum(got.share_ref(k, chrom)[0] > 0 for k in range(len(devices))) > 1]
            for chrom, sub in c.x_kept:
                assert sum(got.share_ref(k, chrom)[0] for k in range(len(devices))) == sub.n
            return cut
    finally:
        got.close()
        want.close()


CASES = [("junctions_u", 11, F.FILTER_A), ("random_a", 12, F.FILTER_B), ("random_b", 13, F.FILTER_A)]


@pytest.mark.parametrize("case,seed,filt", CASES)
def test_device_decode_under_a_filter_leaves_the_prefiltered_file(case, seed, filt, ctx, tmp_path, monkeypatch):
    c = F.Case(case, seed, filt, repeat=6)
    x, kept = c.write(str(tmp_path / "f"), with_seq=True)       # (a few dozen BGZF blocks)
    assert os.path.getsize(x) > 0
    _same_files(c, x, kept, ctx)
    for window in ("2", "3", "7"):     # records straddle windows; dropped records lie at block and window edges
        monkeypatch.setenv("SPL_INFLATE_WINDOW_BLOCKS", window)
        _same_files(c, x, kept, ctx)
    monkeypatch.setenv("SPL_EXTRACT_WALK", "1")      # the walking extraction decides about every record again
    _same_files(c, x, kept, ctx)
    monkeypatch.delenv("SPL_INFLATE_WINDOW_BLOCKS")
    _same_files(c, x, kept, ctx)


@pytest.mark.parametrize("walk", [False, True])
def test_device_decode_in_shares_under_a_filter(walk, ctx, tmp_path, monkeypatch):
    """Three shares on one physical GPU (three contexts), cut at any block: a reference lies across shares, each share counts what
    it drops, the sums are the file's."""
    if walk:
        monkeypatch.setenv("SPL_EXTRACT_WALK", "1")
    c = F.Case("junctions_u", 21, F.FILTER_A, repeat=8)
    x, kept = c.write(str(tmp_path / "s"), with_seq=True)
    cut = _same_files(c, x, kept, ctx, devices=(0, 0, 0))
    assert cut, "no reference was cut across shares"
    monkeypatch.setenv("SPL_INFLATE_WINDOW_BLOCKS", "3")
    _same_files(c, x, kept, ctx, devices=(0, 0, 0))


@pytest.mark.parametrize("walk", [False, True])
def test_blocks_in_which_every_record_is_dropped(walk, ctx, tmp_path, monkeypatch):
    """The first reference's reads all fail (MAPQ 0, supplementary): the file begins with several whole BGZF blocks without a placed
    record, and the block the next reference begins in has them in its first half."""
    if walk:
        monkeypatch.setenv("SPL_EXTRACT_WALK", "1")
    c = F.Case("combine_a/sample0", 31, F.FILTER_A, repeat=8)
    names = c.names
    assert len(names) >= 2
    c = F.Case("combine_a/sample0", 31, F.FILTER_A, repeat=8, all_fail=names[0])
    x, kept = c.write(str(tmp_path / "b"), with_seq=True)
    assert c.x_kept[0][1].n == 0 and c.x[0][1].n * 250 > 3 * 65536
    _same_files(c, x, kept, ctx)
    monkeypatch.setenv("SPL_INFLATE_WINDOW_BLOCKS", "2")
    _same_files(c, x, kept, ctx)
    _same_files(c, x, kept, ctx, devices=(0, 0, 0))


def test_a_file_in_which_every_record_is_dropped(ctx, tmp_path, capsys, oracle_lib):
    c = F.Case("junctions_u", 11, F.FILTER_A, repeat=3)
    x, _ = c.write(str(tmp_path / "e"), with_seq=True)
    for devices in (None, (0, 0, 0)):
        bam = _decode(x, ctx, (255, 0x8000, 0), devices)   # (no read has bit 0x8000: all go by their flags)
        for chrom, _ in c.x:
            assert bam.wait_ref(chrom)[0] == 0
            r = bam.reads(chrom)
            assert r is None or r.n == 0
        assert bam.filter_counts() == (c.n_all, 0) and bam.n_records == c.n_all
        bam.close()
    # ... and the commands: a header and no rows, no junctions; not an error
    prefix = str(tmp_path / "none")
    bed = os.path.join(c.dir, "junctions.bed")
    assert cli.main(["process", "-B", x, "-b", bed, "-o", prefix, "--requireFlags", "0x8000"]) == 0
    nothing = types.SimpleNamespace(genome=types.SimpleNamespace(chrom_names=list(c.names)), reads=[samio.ReadSet.empty() for _ in c.names])
    assert open(prefix + ".SpliSER.tsv").read() == _oracle_tsv(oracle_lib, bed, nothing, None, False)
    assert "dropped by flags" in capsys.readouterr().out
    assert cli.main(["junctions", "-B", x, "-o", prefix + ".bed", "--requireFlags", "0x8000"]) == 0
    assert [line for line in open(prefix + ".bed") if not line.startswith("track")] == []


def _workload(c, kept):
    sets = dict(c.x_kept if kept else c.x)
    return types.SimpleNamespace(genome=types.SimpleNamespace(chrom_names=list(c.names)), reads=[sets.get(n, samio.ReadSet.empty()) for n in c.names])


@pytest.mark.parametrize("case,seed,filt,argv,stranded,cryptic", [
    ("junctions_u", 11, F.FILTER_A, [], None, False),
    ("random_a", 12, F.FILTER_B, ["--isStranded", "-s", "fr"], "fr", False),
    ("random_b", 13, F.FILTER_A, ["--isStranded", "-s", "fr", "--beta2Cryptic"], "fr", True),
])
def test_process_with_the_flags_writes_what_the_prefiltered_file_gives(case, seed, filt, argv, stranded, cryptic, tmp_path, oracle_lib, capsys):
    c = F.Case(case, seed, filt, repeat=2)
    c.assert_beta1_differs(oracle_lib, stranded)
    x, kept = c.write(str(tmp_path / "p"), with_seq=True)
    bed = os.path.join(c.dir, "junctions.bed")
    out = lambda tag: str(tmp_path / tag)      # noqa: E731
    tsv = lambda tag: open(out(tag) + ".SpliSER.tsv").read()      # noqa: E731
    # with a junction file: device decode, host decode, in shares
    want = _oracle_tsv(oracle_lib, bed, _workload(c, True), stranded, cryptic)
    assert want != _oracle_tsv(oracle_lib, bed, _workload(c, False), stranded, cryptic)
    for tag, extra in (("dev", []), ("host", ["--hostDecode"]), ("shares", ["--devices", "0,0,0"])):
        assert cli.main(["process", "-B", x, "-b", bed, "-o", out(tag)] + argv + _flags(filt) + extra) == 0
        assert "dropped by flags, %d dropped by MAPQ" % c.by_mapq in capsys.readouterr().out
        assert cli.main(["process", "-B", kept, "-b", bed, "-o", out(tag + "_kept")] + argv + extra) == 0
        assert tsv(tag) == tsv(tag + "_kept") == want, tag
    # all three at zero: the run without the flags
    assert cli.main(["process", "-B", x, "-b", bed, "-o", out("zero")] + argv + _flags((0, 0, 0))) == 0
    assert cli.main(["process", "-B", x, "-b", bed, "-o", out("bare")] + argv) == 0
    assert tsv("zero") == tsv("bare") == _oracle_tsv(oracle_lib, bed, _workload(c, False), stranded, cryptic)
    # without one: the junctions are those of the reads that pass, the BED that of X'
    knobs = ["--minAnchor", "1", "--minIntron", "1", "--maxIntron", "0", "--keepJunctions"]
    for tag, extra in (("nb", []), ("nb_host", ["--hostDecode"])):
        assert cli.main(["process", "-B", x, "-o", out(tag)] + argv + knobs + _flags(filt) + extra) == 0
        assert cli.main(["process", "-B", kept, "-o", out(tag + "_kept")] + argv + knobs + extra) == 0
        assert tsv(tag) == tsv(tag + "_kept"), tag
        assert open(out(tag) + ".junctions.bed").read() == open(out(tag + "_kept") + ".junctions.bed").read(), tag
        assert tsv(tag) == _oracle_tsv(oracle_lib, out(tag + "_kept") + ".junctions.bed", _workload(c, True), stranded, cryptic), tag
    assert cli.main(["process", "-B", x, "-o", out("nb_zero")] + argv + knobs + _flags((0, 0, 0))) == 0
    assert cli.main(["process", "-B", x, "-o", out("nb_bare")] + argv + knobs) == 0
    assert tsv("nb_zero") == tsv("nb_bare") and tsv("nb_bare") != tsv("nb")
    assert open(out("nb_zero") + ".junctions.bed").read() == open(out("nb_bare") + ".junctions.bed").read()
    # the junctions command
    jk = ["-a", "1", "-m", "1", "-M", "0"] + [a for a in argv if a != "--beta2Cryptic"]
    assert cli.main(["junctions", "-B", x, "-o", out("j.bed")] + jk + _flags(filt)) == 0
    assert cli.main(["junctions", "-B", kept, "-o", out("j_kept.bed")] + jk) == 0
    assert cli.main(["junctions", "-B", x, "-o", out("j_bare.bed")] + jk) == 0
    assert cli.main(["junctions", "-B", x, "-o", out("j_zero.bed")] + jk + _flags((0, 0, 0))) == 0
    assert open(out("j.bed")).read() == open(out("j_kept.bed")).read() == open(out("nb") + ".junctions.bed").read()
    assert open(out("j_bare.bed")).read() == open(out("j_zero.bed")).read() != open(out("j.bed")).read()


def test_check_junctions_compares_with_the_filtered_reads(tmp_path):
    c = F.Case("junctions_u", 11, F.FILTER_A)
    x, kept = c.write(str(tmp_path / "c"), with_seq=True)
    bed = os.path.join(c.dir, "junctions.bed")
    assert cli.main(["process", "-B", x, "-b", bed, "-o", str(tmp_path / "a"), "--checkJunctions"] + _flags(c.filt)) == 0
    assert cli.main(["process", "-B", kept, "-b", bed, "-o", str(tmp_path / "b"), "--checkJunctions"]) == 0
    assert open(str(tmp_path / "a.junctionCheck.tsv")).read() == open(str(tmp_path / "b.junctionCheck.tsv")).read()


@pytest.mark.parametrize("command,extra", [("combine", []), ("combineShallow", ["-m", "1", "-r", "1"])])
def test_kept_reads_and_combine_under_a_filter(command, extra, tmp_path, capsys, monkeypatch):
    """process --keepReads under a filter, then combine under the same one: the combined file of the pre-filtered samples, with the
    kept reads taken and with them gone; under another filter the kept reads are ignored and the file is that filter's."""
    cases = [F.Case("combine_a/sample%d" % k, 40 + k, F.FILTER_A) for k in range(3)]
    d = str(tmp_path)

    def samples(tag, bams, flags, keep=False):
        lines = []
        for k, (c, bam) in enumerate(zip(cases, bams)):
            prefix = os.path.join(d, "%s_s%d" % (tag, k))
            assert cli.main(["process", "-B", bam, "-b", os.path.join(c.dir, "junctions.bed"), "-o", prefix] + flags + (["--keepReads"] if keep else [])) == 0
            lines.append("S%d\t%s.SpliSER.tsv\t%s\n" % (k, prefix, bam))
        path = os.path.join(d, tag + ".samples.tsv")
        with open(path, "w") as fh:
            fh.writelines(lines)
        return path

    def combined(tag, samples_file, flags):
        capsys.readouterr()
        assert cli.main([command, "-S", samples_file, "-o", os.path.join(d, tag)] + extra + flags) == 0
        return open(os.path.join(d, tag + ".combined.tsv")).read(), capsys.readouterr().out

    written = [c.write(os.path.join(d, "in%d" % k), with_seq=True) for k, c in enumerate(cases)]
    xs, kepts = [w[0] for w in written], [w[1] for w in written]
    want, _ = combined("want", samples("want", kepts, []), [])
    s_x = samples("x", xs, _flags(F.FILTER_A), keep=True)
    got, said = combined("got", s_x, _flags(F.FILTER_A))
    assert got == want and said.count("reads kept by process") == 3
    # another filter: the kept reads are not its reads -- every BAM is decoded again, and the gaps are filled by that filter's rule
    kept_b = []
    for k, c in enumerate(cases):
        masks = [F.keep_mask(rs.flag, m, F.FILTER_B)[0] for (_, rs), m in zip(c.x, c.mapq)]
        path = os.path.join(d, "kept_b%d.bam" % k)
        samio.write_bam(path, c.names, c.lengths, [(n, F.subset(rs, m)) for (n, rs), m in zip(c.x, masks)], mapq=[q[m] for q, m in zip(c.mapq, masks)], with_seq=True)
        kept_b.append(path)
    # (the samples' own rows are what process wrote under filter A; only the gap fill runs under B: the same rows + the BAMs filtered by B)
    lines = open(s_x).read().splitlines()
    s_b = os.path.join(d, "b.samples.tsv")
    with open(s_b, "w") as fh:
        fh.writelines("%s\t%s\t%s\n" % (ln.split("\t")[0], ln.split("\t")[1], kept_b[k]) for k, ln in enumerate(lines))
    monkeypatch.setenv("SPL_IGNORE_KEPT_READS", "1")
    want_b, _ = combined("want_b", s_b, [])
    monkeypatch.delenv("SPL_IGNORE_KEPT_READS")
    got_b, said = combined("got_b", s_x, _flags(F.FILTER_B))
    assert got_b == want_b and "reads kept by process" not in said
    got_none, said = combined("got_none", s_x, [])          # (and without a filter: not the unfiltered reads either)
    assert "reads kept by process" not in said
    # the kept reads gone: the BAMs again, under the filter
    for k in range(3):
        os.remove(os.path.join(d, "x_s%d.SpliSER.reads" % k))
    again, said = combined("again", s_x, _flags(F.FILTER_A))
    assert again == want and "reads kept by process" not in said
    zero, _ = combined("zero", s_x, _flags((0, 0, 0)))
    assert zero == got_none
