"""Compressed SAM text without a GPU: ``native.SamFile`` on every case of samcases.py written as BGZF (deflated and stored) and as
gzip (one member, two members cut inside a line), decoded by the host parser, must give what the plain text of the same case gives
and what the restatement says -- arrays, counters, flagstat words, the decline's line and reason; headers cut by block edges;
``open_alignments``' routing by what the first member inflates to; ``read_sam`` on compressed goldens; damaged files; and the
inflate-and-carry parser in a sanitizer build of its own."""
import glob
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import samcases as S
import samzcases as Z
from samzcases import snapshot
from spliser_amd import native, samio
from test_samcases_host import open_host, same_reads, set_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCEPTED = S.accepted_cases()
DECLINES = S.decline_cases()
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "**", "reads.sam"), recursive=True))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    native.build()


def check_against_reference(sam, case):
    ref = S.reference(case)
    assert sam.declined() == ""
    assert sam.ref_names == case.ref_names and sam.any_order
    assert sam.n_records == ref.n_records and list(sam.filter_counts()) == ref.dropped
    assert np.array_equal(sam.flagstat(), ref.flagstat)
    assert sam.any_order_sorted()[0] == (len(ref.pos) if ref.unordered else 0)
    for name in case.ref_names[:40] + case.ref_names[-3:]:
        assert sam.wait_ref(name) == (len(ref.per_ref[name]["pos"]), ref.per_ref[name]["max_end"])
        same_reads(sam.reads(name), ref.per_ref[name], "%s %s" % (case.name, name[:20]))


@pytest.mark.parametrize("case", ACCEPTED, ids=lambda c: c.name)
def test_host_parser_on_compressed_text_equals_plain_text_and_the_restatement(case, tmp_path, monkeypatch):
    set_window(case, monkeypatch)
    plain = open_host(case, case.write(tmp_path / "x.sam"))
    try:
        assert native.lib().spl_bam_text_compression(plain._h) == 0 and plain.compression == ""
        want = snapshot(plain, case)
    finally:
        plain.close()
    for form, make in Z.FORMS.items():
        sam = open_host(case, Z.write(tmp_path / (form + ".sam.gz"), make(case)))
        try:
            assert sam.compression == Z.KIND[form], form
            assert native.lib().spl_bam_is_text(sam._h) == 1
            check_against_reference(sam, case)
            assert snapshot(sam, case) == want, form
            assert not sam.on_device and sam.blocks_inflated == 0
        finally:
            sam.close()


@pytest.mark.parametrize("case,line_no,reason", DECLINES, ids=lambda v: v.name if isinstance(v, S.Case) else None)
def test_declined_with_the_plain_texts_line_number(case, line_no, reason, tmp_path, monkeypatch):
    set_window(case, monkeypatch)
    for form, make in Z.FORMS.items():
        sam = open_host(case, Z.write(tmp_path / (form + ".sam.gz"), make(case)))
        try:
            assert sam.declined() == "line %d %s" % (line_no, S.REASON_TEXT[reason]), form
            with pytest.raises(native.SpliserNativeError) as err:
                sam.wait_ref(case.ref_names[0])
            assert err.value.code == -5 and "line %d " % line_no in str(err.value)
        finally:
            sam.close()


def test_a_header_over_three_blocks_and_an_sq_line_cut_by_a_block_edge(tmp_path):
    case = [c for c in ACCEPTED if c.name == "names"][0]         # (a thousand @SQ lines)
    text = case.text()
    sq = text.index(b"@SQ\tSN:scaffold_500\t") + 9               # inside the name of an @SQ line
    ln_at = text.index(b"LN:", text.index(b"@SQ\tSN:scaffold_900\t")) + 5   # inside the digits of an LN
    assert sq < ln_at < case.begin
    for form, data in (("bgzf", Z.bgzf(text, [sq, ln_at, case.begin + 40])), ("bgzf_small", Z.bgzf(text, block=300)), ("gzip", Z.gz(text, [sq, ln_at]))):
        sam = open_host(case, Z.write(tmp_path / (form + ".sam.gz"), data))
        try:
            assert sam.ref_names == case.ref_names, form
            assert sam.ref_lengths == [case.ref_len] * len(case.ref_names)
            check_against_reference(sam, case)
        finally:
            sam.close()
    # the header's refusals are the plain text's
    for bad in (b"@HD\tVN:1.6\n" + b"\n".join(case.lines[:3]) + b"\n", b"@SQ\tSN:chr1\tLN:5\n@SQ\tSN:chr1\tLN:5\n", b"@SQ\tSN:chr1\n", b"@SQ\tSN:chr1\tLN:5\n@SQX\tSN:chr9\n"):
        for data in (Z.bgzf(bad, block=7), Z.gz(bad)):
            with pytest.raises(native.SpliserNativeError) as err:
                native.SamFile(Z.write(tmp_path / "bad.sam.gz", data))
            assert err.value.code == -5


def test_what_the_opening_calls_refuse(tmp_path):
    case = ACCEPTED[0]
    twin = S.write_twin(case, tmp_path / "x.bam")
    with pytest.raises(native.SpliserNativeError) as err:
        native.SamFile(twin)                                     # a real BAM is spl_bam_open's
    assert err.value.code == -5
    garbage = Z.write(tmp_path / "garbage.gz", Z.gz(bytes(range(256)) * 40))
    with pytest.raises(native.SpliserNativeError) as err:
        native.SamFile(garbage)                                  # gzip data that is neither BAM nor SAM text
    assert err.value.code == -5
    for form in ("bgzf1", "gzip1"):                              # spl_bam_open* keep refusing text of either kind
        path = Z.write(tmp_path / (form + ".sam.gz"), Z.FORMS[form](case))
        for kw in (dict(), dict(defer=True), dict(stream=True)):
            with pytest.raises(native.SpliserNativeError) as err:
                native.BamFile(path, **kw)
            assert err.value.code == -5
    # BGZF without its EOF marker: truncated, as for a BAM
    with pytest.raises(native.SpliserNativeError, match="EOF marker missing") as err:
        native.SamFile(Z.write(tmp_path / "noeof.sam.gz", Z.bgzf(case.text(), eof=False)))
    assert err.value.code == -4
    sam = native.SamFile(Z.write(tmp_path / "ok.sam.gz", Z.FORMS["bgzf1"](case)))
    try:
        for call in (sam.compression_ratio, sam.sample, lambda: sam.decode_on_devices_async([0])):
            with pytest.raises(native.SpliserNativeError) as err:
                call()
            assert err.value.code == -1 and "text" in str(err.value)
        assert sam.wait_all() is True
    finally:
        sam.close()


def test_damaged_data_ends_the_decode_with_an_error_not_with_fewer_reads(tmp_path):
    """A block with a wrong CRC32 in its trailer and an intact payload; a gzip member cut short: the opening call takes the file (its
    header is whole), the decode fails, and it is no decline -- nobody reads such a file by other means."""
    case = S.large_case()
    good = Z.bgzf(case.text(), block=0xff00)
    at = good.index(b"\x1f\x8b\x08\x04", len(good) // 2)        # a block in the file's second half
    bsize = struct.unpack("<H", good[at + 16:at + 18])[0] + 1
    bad = bytearray(good)
    bad[at + bsize - 8] ^= 0x01                                  # its CRC32's first byte
    cut = Z.gz(case.text())
    for name, data in (("crc.sam.gz", bytes(bad)), ("cut.sam.gz", cut[:len(cut) * 2 // 3])):
        sam = native.SamFile(Z.write(tmp_path / name, data))
        try:
            with pytest.raises(native.SpliserNativeError) as err:
                sam.declined()
            assert err.value.code == -5 and "corrupt" in str(err.value), name
            assert sam.decline_reason() == ""
        finally:
            sam.close()


def test_open_alignments_routes_by_what_the_first_member_inflates_to(tmp_path):
    from spliser_amd import process as proc
    case = ACCEPTED[0]
    twin = S.write_twin(case, tmp_path / "x.bam")
    src = proc.open_alignments(twin, defer=True)
    try:
        assert type(src) is native.BamFile
    finally:
        src.close()
    for form, kind in (("bgzf1", "BGZF"), ("gzip1", "gzip")):
        path = Z.write(tmp_path / (form + ".sam.gz"), Z.FORMS[form](case))
        src = proc.open_alignments(path, defer=True)
        try:
            assert isinstance(src, native.SamFile) and src.compression == kind
        finally:
            src.close()
        # without a deferred decode the Python reader has the file, as it has plain text
        src = proc.open_alignments(path)
        assert isinstance(src, proc._SamSource) and src.ref_names == case.ref_names
        assert isinstance(proc.open_and_decode(path, (0,), gpuDecode=False), proc._SamSource)
    garbage = Z.write(tmp_path / "garbage.gz", Z.gz(bytes(range(256)) * 40))
    with pytest.raises(native.SpliserNativeError) as err:
        proc.open_alignments(garbage, defer=True)
    assert err.value.code == -5


def test_without_a_context_the_host_thread_inflates_and_parses(tmp_path, monkeypatch):
    from spliser_amd import process as proc

    def no_context(*a, **kw):
        raise native.SpliserNativeError(-2, "no device")
    monkeypatch.setattr(native, "Context", no_context)
    monkeypatch.delenv("SPL_SAM_WINDOW_BYTES", raising=False)
    case = S.shuffled(S.large_case())[0]
    for form, kind in (("bgzf1", "BGZF"), ("gzip2", "gzip")):
        said = []
        src = proc.open_and_decode(Z.write(tmp_path / (form + ".sam.gz"), Z.FORMS[form](case)), (0,), options=proc.DecodeOptions(aux_strand=True), log=said.append)
        try:
            assert isinstance(src, native.SamFile) and not src.on_device
            assert said == ["  (SAM text, %s: %d lines parsed on host threads)" % (kind, len(case.lines)),
                            "  (the alignment file is not in coordinate order: %d reads sorted on host threads)" % len(S.reference(case).pos)]
            same_reads(src.reads("chr10"), S.reference(case).per_ref["chr10"], "chr10")
        finally:
            src.close()
    bad, line_no, reason = DECLINES[0]
    said = []
    src = proc.open_and_decode(Z.write(tmp_path / "y.sam.gz", Z.FORMS["bgzf1"](bad)), (0,), log=said.append)
    assert isinstance(src, proc._SamSource) and said == ["  (SAM text, BGZF: line %d %s: read by the Python reader)" % (line_no, S.REASON_TEXT[reason])]


def _carriage_return_texts():
    """Texts the native decoders decline, so that they always reach ``read_sam``: CRLF line ends behind XS tags, a lone carriage
    return inside a line, and samcases' decline case -- ``open(path, "r")`` ends a line at each of them."""
    head = b"@HD\tVN:1.6\r\n@SQ\tSN:chr1\tLN:100000\r\n@SQ\tSN:chr2\tLN:100000\r\n"
    crlf = head + b"".join(S.ln(q=b"x%d" % k, pos=100 + k, cigar=b"20M100N30M", tags=[b"NH:i:1", b"XS:A:" + (b"+", b"-")[k % 2]]) + b"\r\n" for k in range(6))
    lone = head.replace(b"\r\n", b"\n") + S.ln(pos=5, cigar=b"20M100N30M", tags=[b"XS:A:+"]) + b"\n" + S.ln(pos=6, tags=[b"CO:Z:a\rb"]) + b"\n" + S.ln(pos=7) + b"\r" + S.ln(pos=8, rname=b"chr2") + b"\n"
    case = [c for c, _, _ in DECLINES if c.name == "decline_carriage_return"][0]
    return [("crlf", crlf), ("lone_cr", lone), ("decline_case", case.text())]


def test_read_sam_on_compressed_goldens_equals_read_sam_on_the_text(tmp_path):
    assert len(GOLDEN) == 17
    texts = []
    for path in GOLDEN:
        with open(path, "rb") as fh:
            texts.append((path, fh.read()))
    for name, text in _carriage_return_texts():
        texts.append((Z.write(tmp_path / (name + ".sam"), text), text))
    crlf = samio.read_sam(texts[17][0], aux_strand=True)[1]["chr1"]
    assert crlf.xs.tolist() == [43, 45] * 3, "a CRLF line's last tag is read without its carriage return"
    for k, (path, text) in enumerate(texts):
        plain_counts = [0, 0, 0]
        names, sets = samio.read_sam(path, aux_strand=True, counts=plain_counts)
        for form, data in (("gzip", gzip.compress(text)), ("bgzf", Z.bgzf(text, block=4093)), ("bgzf7", Z.bgzf(text, block=7 if len(text) < 4000 else 997))):
            counts = [0, 0, 0]
            got_names, got = samio.read_sam(Z.write(tmp_path / ("%d.%s.sam.gz" % (k, form)), data), aux_strand=True, counts=counts)
            assert got_names == names and sorted(got) == sorted(sets), (path, form)
            if b"\r" not in text:
                assert counts[0] == sum(1 for line in text.split(b"\n") if line and not line.startswith(b"@"))
            assert counts == plain_counts, (path, form)
            for name in sets:
                for field in ("pos", "flag", "cig_off", "cigar", "xs"):
                    assert np.array_equal(getattr(got[name], field), getattr(sets[name], field)), (path, form, name, field)


def test_the_inflate_and_carry_parser_under_the_sanitizers(tmp_path):
    """tests/hostsim/sam_gz_asan.cpp, a program of its own: the compressed file in a heap block of exactly its size, every line
    through the rule where the walk's buffer holds it; what it prints is what the restatement says, line for line, and its buffer
    never holds more than two windows of text."""
    exe = str(tmp_path / "sam_gz_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostsim", "sam_gz_asan.cpp"), "-o", exe, "-lz"])
    n_lines = 0
    cases = [c for c in ACCEPTED if c.name in ("windows_4k", "line_fills_window", "no_final_newline", "header_only", "long_lines", "many_ops", "large_shuffled", "xs")]
    cases += [c for c, _, _ in DECLINES if c.name in ("decline_long_line", "decline_bad_before_long", "decline_last_line", "decline_empty_line", "decline_carriage_return")]
    assert len(cases) == 13
    for k, case in enumerate(cases):
        names_path = str(tmp_path / ("names%d.bin" % k))
        with open(names_path, "wb") as fh:
            fh.write(struct.pack("<4I", case.filt[0], case.filt[1], case.filt[2], len(case.ref_names)))
            for n in case.ref_names:
                fh.write(struct.pack("<I", len(n)) + n.encode("ascii"))
        tid_of = {n.encode("ascii"): t for t, n in enumerate(case.ref_names)}
        window = case.window or (256 << 20)
        body = case.text()[case.begin:]
        lines = body.split(b"\n")
        if body.endswith(b"\n") or not body:
            lines.pop()
        want = []
        for i, line in enumerate(lines):
            has_nl = i + 1 < len(lines) or body.endswith(b"\n")
            reason, g = (S.R["LONG_LINE"], None) if len(line) + int(has_nl) > window else S.rule(line, tid_of, case.filt)
            if reason:
                want.append("declined %d %d" % (i + 1, reason))
                break
            want.append("0 %d %d %d %d" % (g["flag"], g["tid"], g["pos"], len(g["ops"])))
        for form, make in Z.FORMS.items():
            path = Z.write(tmp_path / ("%d.%s.sam.gz" % (k, form)), make(case))
            out = subprocess.run([exe, path, names_path, str(case.begin), str(window)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                 env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
            assert out.returncode == 0, out.stderr
            got = out.stdout.strip().split("\n")
            end = got.pop().split()
            assert got == want, (case.name, form)
            assert end[0] == "end" and int(end[1]) == (1 if want and want[-1].startswith("declined") else 0)
            assert int(end[2]) <= 2 * max(window, 64), (case.name, form, end)
            n_lines += len(got)
        # a member cut short: the lines in front of the damage, then status -1
        cut = Z.gz(case.text())
        path = Z.write(tmp_path / ("%d.cut.gz" % k), cut[:len(cut) - 9])
        out = subprocess.run([exe, path, names_path, str(case.begin), str(window)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                             env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        assert out.returncode == 0, out.stderr
        end = out.stdout.strip().split("\n")[-1].split()
        assert end[0] == "end" and int(end[1]) in ((-1, 1) if want and want[-1].startswith("declined") else (-1,)), (case.name, end)
    assert n_lines > 4 * 6000
