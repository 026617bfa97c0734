"""The strict rule for SAM text (csrc/spl_sam_line.h) without a GPU: its Python restatement (samcases.py) against ``samio.read_sam``
on every accepted case and every golden ``reads.sam``; ``native.SamFile`` decoded by the host parser against the restatement --
arrays, counters, strand bytes, the order under shuffled lines; its flagstat counters against the host BAM decoder's on the BAM
of the same records; every decline with its line number; and the rule alone in a sanitizer build of its own."""
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

import samcases as S
from spliser_amd import native, samio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCEPTED = S.accepted_cases()
TWINS = [c for c in ACCEPTED if c.twin]
DECLINES = S.decline_cases()
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "**", "reads.sam"), recursive=True))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    native.build()


def same_reads(got, want, what):
    """A ReadSet (or None) against one entry of the restatement's per-reference arrays."""
    if got is None:
        assert len(want["pos"]) == 0, what
        return
    for k in ("pos", "flag", "cig_off", "cigar"):
        assert np.array_equal(getattr(got, k), want[k]), "%s: %s" % (what, k)
    if got.n:
        assert got.xs is not None and np.array_equal(got.xs, want["xs"]), "%s: xs" % what
        assert got.max_end == want["max_end"], "%s: max_end" % what


@pytest.mark.parametrize("case", ACCEPTED, ids=lambda c: c.name)
def test_restatement_equals_read_sam(case, tmp_path):
    ref = S.reference(case)
    assert ref.decline is None
    counts = [0, 0, 0]
    names, sets = samio.read_sam(case.write(tmp_path / "x.sam"), *case.filt, counts=counts, aux_strand=True)
    assert names == case.ref_names
    assert counts == [ref.n_records] + ref.dropped
    for name in case.ref_names:
        same_reads(sets.get(name), ref.per_ref_file[name], "%s %s" % (case.name, name[:20]))


def test_golden_files_are_accepted_and_equal_read_sam():
    """All of tests/golden/**/reads.sam: the rule takes every line, and what it reads is what read_sam reads."""
    assert len(GOLDEN) == 17
    for path in GOLDEN:
        names, sets = samio.read_sam(path, aux_strand=True)
        tid_of = {n.encode("ascii"): k for k, n in enumerate(names)}
        with open(path, "rb") as fh:
            raw = fh.read()
        assert raw.endswith(b"\n")
        per = {n: ([], [], [0], [], []) for n in names}
        for line in raw[:-1].split(b"\n"):
            if line.startswith(b"@"):
                continue
            reason, g = S.rule(line, tid_of)
            assert reason == 0, (path, line[:60], reason)
            if g["placed"]:
                p = per[names[g["tid"]]]
                p[0].append(g["pos"]); p[1].append(g["flag"]); p[3].extend(g["ops"]); p[2].append(len(p[3])); p[4].append(g["xs"])
        for n in names:
            want = dict(zip(("pos", "flag", "cig_off", "cigar", "xs"), (np.asarray(a, np.int64) for a in per[n])))
            got = sets.get(n)
            assert (got.n if got is not None else 0) == len(want["pos"]), (path, n)
            if got is not None:
                for k in want:
                    assert np.array_equal(getattr(got, k).astype(np.int64), want[k]), (path, n, k)


def set_window(case, monkeypatch):
    """SPL_SAM_WINDOW_BYTES as the case asks: the device's windows, and for both decoders the longest line the rule takes."""
    if case.window:
        monkeypatch.setenv("SPL_SAM_WINDOW_BYTES", str(case.window))
    else:
        monkeypatch.delenv("SPL_SAM_WINDOW_BYTES", raising=False)


def open_host(case, path, **kw):
    q, f, F = case.filt
    return native.SamFile(path, min_mapq=q, require_flags=f, exclude_flags=F, aux_strand=True, flagstat=True, **kw)


@pytest.mark.parametrize("case", ACCEPTED, ids=lambda c: c.name)
def test_host_parser_equals_the_restatement(case, tmp_path, monkeypatch):
    ref = S.reference(case)
    set_window(case, monkeypatch)
    sam = open_host(case, case.write(tmp_path / "x.sam"))
    try:
        assert sam.declined() == ""
        assert sam.ref_names == case.ref_names and sam.any_order
        assert sam.n_records == ref.n_records
        assert list(sam.filter_counts()) == ref.dropped
        assert np.array_equal(sam.flagstat(), ref.flagstat)
        assert sam.any_order_sorted() == (len(ref.pos) if ref.unordered else 0, False)
        assert sam.wait_all() is True
        for name in case.ref_names[:40] + case.ref_names[-3:]:
            assert sam.wait_ref(name) == (len(ref.per_ref[name]["pos"]), ref.per_ref[name]["max_end"])
            same_reads(sam.reads(name), ref.per_ref[name], "%s %s" % (case.name, name[:20]))
    finally:
        sam.close()


def test_shuffled_lines_come_out_in_the_order_of_the_sorted_file():
    """The large case shuffled: per reference stable by POS -- for equal POS the order of the shuffled file, which the restatement
    of the shuffled case states; and the same multiset as the file in order."""
    large, shuffled = S.large_case(), S.shuffled(S.large_case())[0]
    a, b = S.reference(large), S.reference(shuffled)
    assert not a.unordered and b.unordered
    for name in large.ref_names:
        assert np.array_equal(np.sort(a.per_ref[name]["pos"]), b.per_ref[name]["pos"])
    assert np.array_equal(a.flagstat, b.flagstat)


@pytest.mark.parametrize("case", TWINS, ids=lambda c: c.name)
def test_counters_equal_the_host_bam_decoder_on_the_twin(case, tmp_path, monkeypatch):
    ref = S.reference(case)
    set_window(case, monkeypatch)
    q, f, F = case.filt
    bam = native.BamFile(S.write_twin(case, tmp_path / "x.bam"), defer=True, min_mapq=q, require_flags=f, exclude_flags=F, aux_strand=True, flagstat=True, any_order=True)
    sam = open_host(case, case.write(tmp_path / "x.sam"))
    try:
        bam.start_host_decode()
        assert sam.declined() == ""
        assert np.array_equal(sam.flagstat(), bam.flagstat())
        assert sam.n_records == bam.n_records == ref.n_records
        assert sam.filter_counts() == bam.filter_counts()
        # text is sorted when reference ids OR POS ever go down, a BAM in any order when its reference ids do: where only the
        # text was sorted, the BAM's reads are put in the same order here (stable by POS) before they are compared
        only_text = bool(sam.any_order_sorted()[0]) and not bam.any_order_sorted()[0]
        for name in case.ref_names[:40]:
            got, want = sam.reads(name), by_pos(bam.reads(name)) if only_text else bam.reads(name)
            for k in ("pos", "flag", "cig_off", "cigar"):
                assert np.array_equal(getattr(got, k), getattr(want, k)), (case.name, name, k)
            if got.n:
                assert np.array_equal(got.xs, want.xs) and got.max_end == want.max_end, (case.name, name)
    finally:
        sam.close()
        bam.close()


def by_pos(rs):
    """The ReadSet's reads stable by POS."""
    order = np.argsort(rs.pos, kind="stable")
    off = rs.cig_off.astype(np.int64)
    ops = [rs.cigar[off[i]:off[i + 1]] for i in order]
    return samio.ReadSet(rs.pos[order], rs.flag[order], np.concatenate(([0], np.cumsum([len(o) for o in ops]))), np.concatenate(ops) if ops else np.zeros(0, np.uint32),
                         max_end=rs.max_end, xs=None if rs.xs is None else rs.xs[order])


@pytest.mark.parametrize("case,line_no,reason", DECLINES, ids=lambda v: v.name if isinstance(v, S.Case) else None)
def test_declined_with_the_line_number(case, line_no, reason, tmp_path, monkeypatch):
    if reason != S.R["LONG_LINE"]:          # (that one is about a line's length against the window, not about its bytes)
        assert S.reference(case).decline == (line_no, reason)
    set_window(case, monkeypatch)
    sam = open_host(case, case.write(tmp_path / "x.sam"))
    try:
        assert sam.declined() == "line %d %s" % (line_no, S.REASON_TEXT[reason])
        with pytest.raises(native.SpliserNativeError) as err:
            sam.wait_ref(case.ref_names[0])
        assert err.value.code == -5 and "line %d " % line_no in str(err.value)
    finally:
        sam.close()


def test_what_the_opening_call_refuses_and_what_text_has_no_answer_for(tmp_path):
    case = ACCEPTED[0]
    twin = S.write_twin(case, tmp_path / "x.bam")
    bare = tmp_path / "bare.sam"
    bare.write_bytes(b"@HD\tVN:1.6\n" + b"\n".join(case.lines) + b"\n")
    twice = tmp_path / "twice.sam"
    twice.write_bytes(b"@SQ\tSN:chr1\tLN:5\n@SQ\tSN:chr1\tLN:5\n")
    no_ln = tmp_path / "no_ln.sam"
    no_ln.write_bytes(b"@SQ\tSN:chr1\n")
    odd_sq = tmp_path / "odd_sq.sam"          # (read_sam takes the SN: of any line that begins "@SQ")
    odd_sq.write_bytes(b"@SQ\tSN:chr1\tLN:5\n@SQX\tSN:chr9\n")
    for path in (twin, bare, twice, no_ln, odd_sq):
        with pytest.raises(native.SpliserNativeError) as err:
            native.SamFile(str(path))
        assert err.value.code == -5
    with pytest.raises(native.SpliserNativeError, match="BGZF"):
        native.BamFile(case.write(tmp_path / "x.sam"))
    sam = native.SamFile(case.write(tmp_path / "x.sam"))
    try:
        assert native.lib().spl_bam_is_text(sam._h) == 1
        for call in (sam.compression_ratio, sam.sample, lambda: sam.decode_on_devices_async([0])):
            with pytest.raises(native.SpliserNativeError) as err:
                call()
            assert err.value.code == -1 and "text" in str(err.value)
        assert sam.wait_all() is True
    finally:
        sam.close()
    bam = native.BamFile(twin)
    assert native.lib().spl_bam_is_text(bam._h) == 0
    bam.close()


def test_open_alignments_keeps_the_python_reader_where_it_was(tmp_path):
    """Without a deferred decode (``--hostDecode``, or a caller that reads the file at once) SAM text is the Python reader's, as
    before: its flagstat error included."""
    from spliser_amd import process as proc
    path = ACCEPTED[0].write(tmp_path / "x.sam")
    assert isinstance(proc.open_alignments(path), proc._SamSource)
    assert isinstance(proc.open_and_decode(path, (0,), gpuDecode=False), proc._SamSource)
    with pytest.raises(native.SpliserNativeError):
        proc.open_alignments(path, options=proc.DecodeOptions(flagstat=True))
    src = proc.open_alignments(path, defer=True, options=proc.DecodeOptions(flagstat=True))
    try:
        assert isinstance(src, native.SamFile) and src.flagstat().shape == (16, 2)
    finally:
        src.close()


def test_without_a_context_the_host_thread_parses_and_a_declined_file_is_the_python_readers(tmp_path, monkeypatch):
    """``open_and_decode`` where no context can be made on the device: the same rule on the host thread, the same log lines, and the
    Python reader for a file the rule declines."""
    from spliser_amd import process as proc

    def no_context(*a, **kw):
        raise native.SpliserNativeError(-2, "no device")
    monkeypatch.setattr(native, "Context", no_context)
    monkeypatch.delenv("SPL_SAM_WINDOW_BYTES", raising=False)
    case = S.shuffled(S.large_case())[0]
    said = []
    src = proc.open_and_decode(case.write(tmp_path / "x.sam"), (0,), options=proc.DecodeOptions(aux_strand=True), log=said.append)
    try:
        assert isinstance(src, native.SamFile) and not src.on_device
        assert said == ["  (SAM text: %d lines parsed on host threads)" % len(case.lines),
                        "  (the alignment file is not in coordinate order: %d reads sorted on host threads)" % len(S.reference(case).pos)]
        same_reads(src.reads("chr10"), S.reference(case).per_ref["chr10"], "chr10")
    finally:
        src.close()
    bad, line_no, reason = DECLINES[0]
    said = []
    src = proc.open_and_decode(bad.write(tmp_path / "y.sam"), (0,), log=said.append)
    assert isinstance(src, proc._SamSource) and said == ["  (SAM text: line %d %s: read by the Python reader)" % (line_no, S.REASON_TEXT[reason])]


def test_the_rule_under_the_sanitizers(tmp_path):
    """The header alone in a program of its own (tests/hostsim/sam_line_asan.cpp): every line of every case in a heap block of
    exactly its size, the names' table likewise; what it prints is what the restatement says."""
    exe = str(tmp_path / "sam_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostsim", "sam_line_asan.cpp"), "-o", exe])
    by_names = {}
    for case, line in S.all_lines():
        by_names.setdefault((tuple(case.ref_names), case.filt), []).append(line)
    n_checked = 0
    for k, ((names, filt), lines) in enumerate(by_names.items()):
        path = str(tmp_path / ("lines%d.bin" % k))
        with open(path, "wb") as fh:
            fh.write(struct.pack("<4I", filt[0], filt[1], filt[2], len(names)))
            for n in names:
                fh.write(struct.pack("<I", len(n)) + n.encode("ascii"))
            fh.write(struct.pack("<I", len(lines)))
            for line in lines:
                fh.write(struct.pack("<I", len(line)) + line)
        out = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        assert out.returncode == 0, out.stderr
        got = out.stdout.strip().split("\n")
        assert len(got) == len(lines)
        tid_of = {n.encode("ascii"): t for t, n in enumerate(names)}
        for line, text in zip(lines, got):
            reason, g = S.rule(line, tid_of, filt)
            if reason:
                assert text == str(reason), (line[:60], text)
            else:
                want = [0, g["flag"], g["tid"], g["pos"], g["mapq"], g["next_tid"], g["verdict"], int(g["placed"]), g["xs"], g["end"], len(g["ops"])] + g["ops"]
                assert [int(v) for v in text.split()] == want, line[:60]
            n_checked += 1
    assert n_checked > 7000 and any(len(line) > 3 * S.CHUNK for _, line in S.all_lines()) and any(line.count(b"1M1N") == 35000 for _, line in S.all_lines())
