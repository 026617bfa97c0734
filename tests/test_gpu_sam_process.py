"""SAM text through the device decoder and the commands: ``SamFile.decode_on_device`` must TAKE every accepted case of samcases.py
(windows forced small, so that lines end windows, arrays regrow and the sort runs) and leave what the restatement says and what
the BAM twin's device decode leaves; ``process`` on golden ``reads.sam`` files writes the golden TSVs byte for byte, with -b and
without; ``--flagstat --keepReads``, ``flagstat`` and ``strandedness`` give what they give on the BAM twin; a declined file is
read by the Python reader, and says so; ``--hostDecode`` keeps the Python reader."""
import os
import sys

import numpy as np
import pytest

import helpers
import samcases as S
from spliser_amd import cli, native
from spliser_amd import process as proc
from test_samcases_host import same_reads

pytestmark = pytest.mark.gpu

ACCEPTED = S.accepted_cases()


@pytest.fixture(scope="module")
def ctx():
    native.build()
    with native.Context(0) as c:
        yield c


def decode(ctx, case, path, monkeypatch, cls=native.SamFile, **kw):
    if case.window:
        monkeypatch.setenv("SPL_SAM_WINDOW_BYTES", str(case.window))
    else:
        monkeypatch.delenv("SPL_SAM_WINDOW_BYTES", raising=False)
    q, f, F = case.filt
    src = cls(path, defer=True, min_mapq=q, require_flags=f, exclude_flags=F, aux_strand=True, flagstat=True, **kw)
    src.decode_on_device(ctx)
    return src


@pytest.mark.parametrize("case", ACCEPTED, ids=lambda c: c.name)
def test_device_decode_is_taken_and_equals_the_restatement_and_the_twin(ctx, case, tmp_path, monkeypatch):
    ref = S.reference(case)
    sam = decode(ctx, case, case.write(tmp_path / "x.sam"), monkeypatch)
    bam = None
    try:
        assert sam.on_device, "handed to the host: %s" % sam.decline_reason()
        assert sam.declined() == "" and sam.decline_reason() == ""
        assert sam.n_records == ref.n_records and list(sam.filter_counts()) == ref.dropped
        assert np.array_equal(sam.flagstat(), ref.flagstat)
        assert sam.any_order_sorted() == (len(ref.pos) if ref.unordered else 0, bool(ref.unordered))
        some = case.ref_names[:40] + case.ref_names[-3:]
        for name in some:
            assert sam.wait_ref(name) == (len(ref.per_ref[name]["pos"]), ref.per_ref[name]["max_end"])
            same_reads(sam.reads(name), ref.per_ref[name], "%s %s" % (case.name, name[:20]))
        if case.twin and ref.unordered == bool(np.any(np.diff(ref.tid) < 0)):     # (a BAM is sorted when its reference ids go down: the same order then)
            bam = decode(ctx, case, S.write_twin(case, tmp_path / "x.bam"), monkeypatch, cls=native.BamFile, any_order=True)
            assert bam.on_device, bam.decline_reason()
            assert np.array_equal(sam.flagstat(), bam.flagstat()) and sam.n_records == bam.n_records and sam.filter_counts() == bam.filter_counts()
            assert sam.any_order_sorted() == bam.any_order_sorted()
            for name in some:
                got, want = sam.reads(name), bam.reads(name)
                for k in ("pos", "flag", "cig_off", "cigar", "xs"):
                    assert np.array_equal(getattr(got, k), getattr(want, k)), (case.name, name, k)
                assert sam.wait_ref(name) == bam.wait_ref(name)
    finally:
        sam.close()
        if bam is not None:
            bam.close()


@pytest.mark.parametrize("case,line_no,reason", S.decline_cases(), ids=lambda v: v.name if isinstance(v, S.Case) else None)
def test_device_decode_declines_with_the_line_number(ctx, case, line_no, reason, tmp_path, monkeypatch):
    sam = decode(ctx, case, case.write(tmp_path / "x.sam"), monkeypatch)
    try:
        assert not sam.on_device
        assert sam.declined() == "line %d %s" % (line_no, S.REASON_TEXT[reason])
    finally:
        sam.close()


def _log_of(fn):
    lines = []
    fn(lines.append)
    return "\n".join(str(m) for m in lines)


def test_process_on_golden_sam_text_writes_the_golden_tsv(tmp_path, monkeypatch):
    sys.path.insert(0, helpers.GOLDEN)
    from make_golden import JUNCTION_KNOBS
    monkeypatch.setenv("SPL_SAM_WINDOW_BYTES", "65536")
    for name, variant, lines in (("kat1", "default", 9), ("cigar_corners", "unstranded", 48), ("multichrom", "noannot", 11), ("junctions_u", "unstranded", 2400)):
        d = os.path.join(helpers.GOLDEN, name)
        out = str(tmp_path / name)
        log = _log_of(lambda say: proc.process(os.path.join(d, "reads.sam"), os.path.join(d, "junctions.bed"), out, log=say))
        assert "(SAM text: %d lines parsed on the GPU)" % lines in log, log
        assert open(out + ".SpliSER.tsv", "rb").read() == open(os.path.join(d, "expected.%s.tsv" % variant), "rb").read(), name
    d = os.path.join(helpers.GOLDEN, "junctions_u")
    out = str(tmp_path / "bedless")
    proc.process(os.path.join(d, "reads.sam"), None, out, log=lambda m: None, **JUNCTION_KNOBS)
    assert open(out + ".SpliSER.tsv", "rb").read() == open(os.path.join(d, "expected.unstranded.tsv"), "rb").read()
    # kat1's lines are not in coordinate order: the decoder says that it sorted them, as for a BAM under --anyOrder
    d = os.path.join(helpers.GOLDEN, "kat1")
    log = _log_of(lambda say: proc.process(os.path.join(d, "reads.sam"), os.path.join(d, "junctions.bed"), str(tmp_path / "again"), log=say))
    assert "(the alignment file is not in coordinate order: 9 reads sorted on the GPU)" in log, log


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """The large case shuffled, as SAM text and as its BAM twin, and a junction file for both."""
    d = tmp_path_factory.mktemp("sam_pair")
    case = S.shuffled(S.large_case())[0]
    sam, bam = case.write(d / "x.sam"), S.write_twin(case, d / "x.bam")
    assert cli.main(["junctions", "-B", bam, "-o", str(d / "j.bed"), "--anyOrder"]) == 0
    return case, sam, bam, str(d / "j.bed")


def test_process_flagstat_and_kept_reads_equal_the_twins(pair, tmp_path, monkeypatch):
    case, sam, bam, bed = pair
    monkeypatch.setenv("SPL_SAM_WINDOW_BYTES", str(case.window))
    outs = {}
    for tag, path in (("sam", sam), ("bam", bam)):
        outs[tag] = str(tmp_path / tag)
        assert cli.main(["process", "-B", path, "-b", bed, "-o", outs[tag], "--flagstat", "--keepReads", "--anyOrder", "--minMapQ", "1"]) == 0
    proc.wait_deferred_close()
    from spliser_amd import flagstat as fstat, readstore
    assert open(outs["sam"] + ".SpliSER.tsv", "rb").read() == open(outs["bam"] + ".SpliSER.tsv", "rb").read()
    assert open(outs["sam"] + fstat.SUFFIX).read() == open(outs["bam"] + fstat.SUFFIX).read()
    kept = {tag: readstore.open_if_fresh(outs[tag] + readstore.SUFFIX, path, read_filter=(1, 0, 0)) for tag, path in (("sam", sam), ("bam", bam))}
    assert kept["sam"] is not None and kept["bam"] is not None and kept["sam"].n_reads == kept["bam"].n_reads > 5000
    for name in case.ref_names:
        a, b = kept["sam"].reads(name), kept["bam"].reads(name)
        for k in ("pos", "flag", "cig_off", "cigar"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), (name, k)


def test_flagstat_and_strandedness_commands_equal_the_twins(pair, tmp_path):
    case, sam, bam, _ = pair
    from spliser_amd import flagstat as fstat
    got = {tag: fstat.flagstat(path, str(tmp_path / (tag + ".flagstat.txt")), anyOrder=True, log=lambda m: None) for tag, path in (("sam", sam), ("bam", bam))}
    assert np.array_equal(got["sam"], got["bam"]) and np.array_equal(got["sam"], S.reference(case).flagstat)
    for tag, path in (("sam", sam), ("bam", bam)):
        assert cli.main(["strandedness", "-B", path, "-o", str(tmp_path / (tag + ".strand.txt")), "--anyOrder"]) == 0
    assert open(str(tmp_path / "sam.strand.txt")).read() == open(str(tmp_path / "bam.strand.txt")).read()


def test_a_declined_file_is_read_by_the_python_reader(tmp_path):
    """kat2's reads and a line the rule does not take (MAPQ 256 on a read without a reference, which read_sam steps over as it
    always did): the Python reader's result, and the log says why."""
    d = os.path.join(helpers.GOLDEN, "kat2")
    raw = open(os.path.join(d, "reads.sam"), "rb").read().rstrip(b"\n").split(b"\n")
    n_header = sum(1 for line in raw if line.startswith(b"@"))
    odd = tmp_path / "odd.sam"
    odd.write_bytes(b"\n".join(raw + [S.ln(flag=4, rname=b"*", pos=0, mapq=256, cigar=b"*")]) + b"\n")
    log = _log_of(lambda say: proc.process(str(odd), os.path.join(d, "junctions.bed"), str(tmp_path / "odd"), log=say))
    assert "(SAM text: line %d %s: read by the Python reader)" % (len(raw) + 1, S.REASON_TEXT[S.R["BAD_MAPQ"]]) in log, log
    assert n_header > 0
    assert open(str(tmp_path / "odd.SpliSER.tsv"), "rb").read() == open(os.path.join(d, "expected.unstranded.tsv"), "rb").read()
    with pytest.raises(native.SpliserNativeError, match="flagstat counters"):
        proc.process(str(odd), os.path.join(d, "junctions.bed"), str(tmp_path / "odd2"), log=lambda m: None, flagstat=True)
    proc.wait_deferred_close()


def test_host_decode_keeps_the_python_reader(tmp_path):
    d = os.path.join(helpers.GOLDEN, "kat2")
    src = proc.open_and_decode(os.path.join(d, "reads.sam"), (0,), gpuDecode=False)
    assert isinstance(src, proc._SamSource)
    log = _log_of(lambda say: proc.process(os.path.join(d, "reads.sam"), os.path.join(d, "junctions.bed"), str(tmp_path / "h"), log=say, gpuDecode=False))
    assert "SAM text" not in log
    assert open(str(tmp_path / "h.SpliSER.tsv"), "rb").read() == open(os.path.join(d, "expected.unstranded.tsv"), "rb").read()
    proc.wait_deferred_close()
