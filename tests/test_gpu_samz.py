"""Compressed SAM text through the device decoder and the commands.  BGZF is inflated on the GPU and parsed where it lies, plain
gzip is inflated by a host thread and parsed by the same kernels; either must leave exactly what the PLAIN-TEXT device decode of the
same text leaves -- the five arrays, the drop counters, the flagstat words, the sort's decision, the decline's line and reason --
wherever BGZF blocks and windows cut the lines: a newline as a block's last and as its first byte, a line over three blocks, an empty
block, a payload of 65 536 bytes, stored blocks; carries chained over windows with the last newline 0..33 bytes in front of the
window's end; a line of exactly a window and one byte more; a line that begins a 16 KiB chunk behind a carry; a wrong CRC32; and
``process`` / ``combine`` on compressed goldens, byte for byte."""
import json
import os
import struct

import numpy as np
import pytest

import helpers
import samcases as S
import samzcases as Z
from spliser_amd import cli, native
from spliser_amd import process as proc
from samzcases import snapshot

pytestmark = pytest.mark.gpu

ACCEPTED = S.accepted_cases()
SHUFFLED = [S.shuffled(c)[0] for c in S.field_cases()[:1] + S.shape_cases()[-2:-1]]


@pytest.fixture(scope="module")
def ctx():
    native.build()
    with native.Context(0) as c:
        yield c


def decode(ctx, case, path, monkeypatch, window=None):
    window = window or case.window
    if window:
        monkeypatch.setenv("SPL_SAM_WINDOW_BYTES", str(window))
    else:
        monkeypatch.delenv("SPL_SAM_WINDOW_BYTES", raising=False)
    q, f, F = case.filt
    src = native.SamFile(path, defer=True, min_mapq=q, require_flags=f, exclude_flags=F, aux_strand=True, flagstat=True)
    before = native.lib().spl_last_error()
    src.decode_on_device(ctx)
    # a device decode that fails (HIP, memory, a bad block) says why and leaves the file to the host parser, which would give the
    # same arrays and the same decline: no test below may pass that way
    src.device_failure = native.lib().spl_last_error() if native.lib().spl_last_error() != before else b""
    return src


_PLAIN = {}


def plain_device(ctx, case, tmp_path, monkeypatch, window=None):
    """What the plain-text device decode of the case leaves (once per case and window)."""
    key = (case.name, window or case.window)
    if key not in _PLAIN:
        sam = decode(ctx, case, case.write(tmp_path / "plain.sam"), monkeypatch, window)
        try:
            assert sam.device_failure == b"", sam.device_failure
            _PLAIN[key] = (snapshot(sam, case), sam.on_device)
            assert sam.on_device == (_PLAIN[key][0]["declined"] == ""), "the device takes what the rule takes"
        finally:
            sam.close()
    return _PLAIN[key]


def same_as_plain(ctx, case, data, tmp_path, monkeypatch, what, window=None, kind="BGZF"):
    want, want_on_device = plain_device(ctx, case, tmp_path, monkeypatch, window)
    sam = decode(ctx, case, Z.write(tmp_path / "x.sam.gz", data), monkeypatch, window)
    try:
        assert sam.compression == kind, what
        assert sam.device_failure == b"", "%s: %s" % (what, sam.device_failure)
        assert want_on_device == (want["declined"] == "")
        assert sam.on_device == want_on_device, "%s: %s / %s" % (what, sam.decline_reason(), native.lib().spl_last_error())
        assert snapshot(sam, case) == want, what
        if kind == "BGZF" and len(case.text()) > case.begin:      # (a text without lines has no block behind its header)
            assert sam.blocks_inflated > 0, "%s: accepted or declined, the device inflated the blocks it judged" % what
    finally:
        sam.close()
    return want


def blocks_of(case, cuts):
    """(first byte, end) of the payloads the device inflates: the blocks that hold anything behind the header."""
    edges = [0] + list(cuts) + [len(case.text())]
    return [(a, b) for a, b in zip(edges, edges[1:]) if b > case.begin]


def windows_of(case, cuts, window):
    """The decoder's windows (csrc/spl_capi.cpp, SamZDecode::plan_z): whole blocks, closed where one more would pass `window` bytes."""
    out, cur = [], []
    for a, b in blocks_of(case, cuts):
        if cur and b - cur[0][0] > window:
            out.append((cur[0][0], cur[-1][1]))
            cur = []
        cur.append((a, b))
    if cur:
        out.append((cur[0][0], cur[-1][1]))
    return out


# ---- block cuts against a line ------------------------------------------------------------------------------------------------
def _forty_lines():
    rng = np.random.default_rng(5)
    lines = [S.fit(1300 + int(rng.integers(0, 400)), q=b"c%d" % k, pos=10 + 3 * k, flag=int(rng.choice([0, 16, 99, 147])), cigar=(b"50M", b"20M100N30M")[k % 2],
                   tags=[b"XS:A:+"] if k % 2 else []) for k in range(40)]
    return S.Case("forty_lines", lines, twin=False)


def test_block_cuts_against_a_line(ctx, tmp_path, monkeypatch):
    case = _forty_lines()
    text, begin = case.text(), case.begin
    assert len(text) > 65536 + 3000
    nls = [i for i in range(begin, len(text)) if text[i:i + 1] == b"\n"]
    a, b, c = nls[5], nls[11], nls[20]
    mid = [nls[25] + 100, nls[25] + 500, nls[25] + 900]           # three cuts inside line 26: its middle block holds no newline
    assert text[mid[0]:mid[1]].count(b"\n") == 0 and mid[2] < nls[26]
    shapes = {
        "newline_last_byte_of_a_block": [begin, a + 1, c + 1],
        "newline_first_byte_of_a_block": [begin, a, b, c],
        "a_block_without_a_newline": [begin] + mid,
        "an_empty_block_mid_file": [begin, a + 7, a + 7, b + 1, b + 1, c],
        "a_payload_of_65536_bytes": [65536],
        "header_and_lines_in_one_block": [begin + 333, c + 2],
    }
    for name, cuts in shapes.items():
        data = Z.bgzf(text, cuts, level=1)
        if name == "a_payload_of_65536_bytes":
            bsize = struct.unpack("<H", data[16:18])[0] + 1
            assert struct.unpack("<I", data[bsize - 4:bsize])[0] == 65536, "the first block's ISIZE"
        want = same_as_plain(ctx, case, data, tmp_path, monkeypatch, name)
        assert want["declined"] == "" and want["n"] == 40
    # stored blocks (level 0): no Huffman code at all
    same_as_plain(ctx, case, Z.bgzf(text, [begin, a + 1, b, c + 3], level=0), tmp_path, monkeypatch, "stored blocks")
    same_as_plain(ctx, case, Z.bgzf(text, level=0, block=4093), tmp_path, monkeypatch, "stored blocks of 4093 bytes")


# ---- window cuts -----------------------------------------------------------------------------------------------------------------
def _sixty_lines():
    rng = np.random.default_rng(9)
    lines = [S.fit(640 + int(rng.integers(0, 120)), q=b"w%d" % k, pos=10 + k, flag=int(rng.choice([0, 16, 99, 147])), cigar=(b"50M", b"20M100N30M", b"25M2I23M")[k % 3]) for k in range(60)]
    return S.Case("sixty_lines", lines, window=4096, twin=False)


def test_carries_chain_over_windows_at_every_distance_from_the_last_newline(ctx, tmp_path, monkeypatch):
    case = _sixty_lines()
    text, begin = case.text(), case.begin
    # blocks of 1000 bytes from the first line on: windows of four blocks, each ending inside a line
    cuts = list(range(begin, len(text), 1000))
    wins = windows_of(case, cuts, 4096)
    assert len(wins) >= 9 and all(text[e - 1:e] != b"\n" for _, e in wins[:-1]), "every window hands a carry to the next"
    same_as_plain(ctx, case, Z.bgzf(text, cuts), tmp_path, monkeypatch, "blocks of 1000 bytes")
    # ... and the first window's end d bytes behind a newline, d = 0 .. 33: every residue of the 16-byte alignment, twice
    nl = max(i for i in range(begin + 3200, begin + 4000) if text[i:i + 1] == b"\n")
    for d in range(34):
        end0 = nl + 1 + d
        cuts = [begin, begin + 1000, begin + 2000, begin + 3000, end0] + list(range(end0 + 1000, len(text), 1000))
        wins = windows_of(case, cuts, 4096)
        assert wins[0] == (begin, end0) and len(wins) >= 9
        same_as_plain(ctx, case, Z.bgzf(text, cuts), tmp_path, monkeypatch, "window ends %d bytes behind a newline" % d)
    # the same text as gzip: the host thread's pieces end at 4096 bytes of text, wherever that is
    same_as_plain(ctx, case, Z.gz(text), tmp_path, monkeypatch, "gzip", kind="gzip")


# ---- line length limits --------------------------------------------------------------------------------------------------------
def test_a_line_of_a_window_is_taken_and_one_byte_more_is_declined_with_the_plain_texts_line(ctx, tmp_path, monkeypatch):
    W = 4096
    ok = [S.ln(pos=5), S.ln(pos=6)]
    cases = [
        (S.Case("exactly_a_window", ok + [S.fit(W, pos=7), S.ln(pos=8)], window=W, twin=False), ""),
        (S.Case("a_window_and_a_byte", ok + [S.fit(W + 1, pos=7), S.ln(pos=8)], window=W, twin=False), "LONG_LINE"),
        (S.Case("last_line_bare", ok + [S.fit(W - 700, pos=7), S.fit(W + 1, pos=8)[:W]], window=W, final_nl=False, twin=False), ""),          # W bytes, no newline
        (S.Case("last_line_bare_too_long", ok + [S.fit(W - 700, pos=7), S.fit(W + 2, pos=8)[:W + 1]], window=W, final_nl=False, twin=False), "LONG_LINE"),
        (S.Case("bad_line_before_the_long_one", ok + [S.ln(flag=b"x"), S.fit(W + 1, pos=7)], window=W, twin=False), "BAD_FLAG"),
        (S.Case("a_line_of_three_windows", ok + [S.fit(3 * W, pos=7), S.ln(pos=8)], window=W, twin=False), "LONG_LINE"),
    ]
    for case, reason in cases:
        for block in (1000, 997, 4096):
            want = same_as_plain(ctx, case, Z.bgzf(case.text(), [case.begin] + list(range(case.begin + block, len(case.text()), block))), tmp_path, monkeypatch,
                                 "%s, blocks of %d" % (case.name, block))
            if reason == "":
                assert want["declined"] == "", case.name
            else:
                assert want["declined"] == "line %d %s" % (case.header_lines + 3 + (reason == "LONG_LINE" and "last" in case.name), S.REASON_TEXT[S.R[reason]]), case.name
        same_as_plain(ctx, case, Z.gz(case.text(), [Z.mid_line_cut(case)]), tmp_path, monkeypatch, case.name + ", gzip", kind="gzip")


# ---- a line that begins a 16 KiB chunk behind a carry -----------------------------------------------------------------------------
def test_a_line_on_the_first_byte_of_a_chunk_behind_a_carry(ctx, tmp_path, monkeypatch):
    W, lead = 32768, 9
    lines = [S.fit(20007, pos=5), S.fit(S.CHUNK, pos=6), S.fit(700, pos=7), S.fit(S.CHUNK - 700, pos=8), S.ln(pos=9), S.fit(5000, pos=10)]
    case = S.Case("chunk_edge", lines, window=W, lead=lead, twin=False)
    text, begin = case.text(), case.begin
    cuts = list(range(begin, len(text), 1000))
    wins = windows_of(case, cuts, W)
    lo1 = begin + 20007                       # where the second window's lines begin: its carry is the front of the 16 KiB line
    assert wins[0][1] == begin + 32000 and lo1 < wins[0][1] < lo1 + S.CHUNK and lo1 % 16 == 0
    assert text[lo1 + S.CHUNK - 1:lo1 + S.CHUNK] == b"\n", "the next line begins on the first byte of the second chunk of that window's lines"
    want = same_as_plain(ctx, case, Z.bgzf(text, cuts), tmp_path, monkeypatch, "chunk edge")
    assert want["declined"] == "" and want["n"] == 6
    same_as_plain(ctx, case, Z.gz(text), tmp_path, monkeypatch, "chunk edge, gzip", kind="gzip")


# ---- every case ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ACCEPTED + SHUFFLED, ids=lambda c: c.name)
def test_every_accepted_case_equals_its_plain_text_device_decode(ctx, case, tmp_path, monkeypatch):
    for form, make in Z.FORMS.items():
        want = same_as_plain(ctx, case, make(case), tmp_path, monkeypatch, "%s %s" % (case.name, form), kind=Z.KIND[form])
        assert want["declined"] == ""
        ref = S.reference(case)
        assert want["n"] == ref.n_records and want["dropped"] == ref.dropped and want["sorted"] == (len(ref.pos) if ref.unordered else 0, bool(ref.unordered))


@pytest.mark.parametrize("case,line_no,reason", S.decline_cases(), ids=lambda v: v.name if isinstance(v, S.Case) else None)
def test_every_declined_case_declines_as_its_plain_text(ctx, case, line_no, reason, tmp_path, monkeypatch):
    for form, make in Z.FORMS.items():
        want = same_as_plain(ctx, case, make(case), tmp_path, monkeypatch, "%s %s" % (case.name, form), kind=Z.KIND[form])
        assert want["declined"] == "line %d %s" % (line_no, S.REASON_TEXT[reason])


# ---- a wrong CRC32 -----------------------------------------------------------------------------------------------------------------
def test_a_block_with_a_wrong_crc_publishes_nothing_and_ends_in_the_host_paths_error(ctx, tmp_path, monkeypatch):
    case = S.large_case()
    good = Z.bgzf(case.text(), block=0xff00)
    at = good.index(b"\x1f\x8b\x08\x04", len(good) // 2)
    bsize = struct.unpack("<H", good[at + 16:at + 18])[0] + 1
    bad = bytearray(good)
    bad[at + bsize - 8] ^= 0x01                  # the CRC32 of the block's trailer; its payload is intact
    sam = decode(ctx, case, Z.write(tmp_path / "crc.sam.gz", bytes(bad)), monkeypatch)
    try:
        assert not sam.on_device
        with pytest.raises(native.SpliserNativeError) as err:
            sam.declined()
        assert err.value.code == -5 and "corrupt" in str(err.value)
        for name in case.ref_names:
            with pytest.raises(native.SpliserNativeError):
                sam.reads(name)
    finally:
        sam.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _log_of(fn):
    lines = []
    fn(lines.append)
    return "\n".join(str(m) for m in lines)


def _packed(path, tmp_path, name, form):
    with open(path, "rb") as fh:
        text = fh.read()
    return Z.write(tmp_path / name, Z.bgzf(text, block=4093) if form == "BGZF" else Z.gz(text, [len(text) // 2]))


def test_process_on_compressed_goldens_writes_the_golden_tsv(tmp_path, monkeypatch):
    monkeypatch.setenv("SPL_SAM_WINDOW_BYTES", "65536")
    for name, variant, lines in (("kat1", "default", 9), ("cigar_corners", "unstranded", 48), ("multichrom", "noannot", 11), ("junctions_u", "unstranded", 2400)):
        d = os.path.join(helpers.GOLDEN, name)
        for form in ("BGZF", "gzip"):
            path = _packed(os.path.join(d, "reads.sam"), tmp_path, "%s.%s.sam.gz" % (name, form), form)
            out = str(tmp_path / (name + form))
            log = _log_of(lambda say: proc.process(path, os.path.join(d, "junctions.bed"), out, log=say))
            if form == "BGZF":
                assert "(SAM text, BGZF: %d lines parsed on the GPU, " % lines in log and " blocks inflated there)" in log, log
                said = int(log.split("lines parsed on the GPU, ")[1].split(" blocks")[0])
                n_blocks = -(-os.path.getsize(os.path.join(d, "reads.sam")) // 4093) + 1      # (payloads of 4093 bytes, and the EOF marker)
                assert 2 <= said <= n_blocks, (said, n_blocks)      # (the blocks of nothing but header are inflated by the opening call alone)
            else:
                assert "(SAM text, gzip: %d lines parsed on the GPU, inflated on one host thread)" % lines in log, log
            assert open(out + ".SpliSER.tsv", "rb").read() == open(os.path.join(d, "expected.%s.tsv" % variant), "rb").read(), (name, form)
    proc.wait_deferred_close()


def test_combine_over_compressed_samples_equals_its_golden(tmp_path):
    case = os.path.join(helpers.GOLDEN, "combine_a")
    manifest = json.load(open(os.path.join(case, "combine_manifest.json")))
    variant = "unstranded"
    sfile = str(tmp_path / "samples.tsv")
    with open(sfile, "w") as fh:
        for k in range(manifest["n_samples"]):
            sd = os.path.join(case, "sample%d" % k)
            packed = _packed(os.path.join(sd, "reads.sam"), tmp_path, "s%d.sam.gz" % k, "BGZF" if k % 2 == 0 else "gzip")
            fh.write("S%d\t%s\t%s\n" % (k, os.path.join(sd, "expected.%s.tsv" % variant), packed))
    v = manifest["variants"][variant]
    assert cli.main([v.get("command", "combine"), "-S", sfile, "-o", str(tmp_path / "all")] + v["combine"]) == 0
    assert open(str(tmp_path / "all.combined.tsv")).read() == open(os.path.join(case, "expected.%s.combined.tsv" % variant)).read()


def test_flagstat_kept_reads_and_a_filter_equal_the_plain_text_run_file_for_file(tmp_path, monkeypatch):
    case = S.shuffled(S.large_case())[0]
    monkeypatch.setenv("SPL_SAM_WINDOW_BYTES", str(case.window))
    sam = case.write(tmp_path / "x.sam")
    assert cli.main(["junctions", "-B", sam, "-o", str(tmp_path / "j.bed")]) == 0
    outs = {}
    for tag, path in (("plain", sam), ("bgzf", Z.write(tmp_path / "b.sam.gz", Z.bgzf(case.text(), block=0xff00, level=6))), ("gzip", Z.write(tmp_path / "g.sam.gz", Z.gz(case.text())))):
        outs[tag] = str(tmp_path / tag)
        assert cli.main(["process", "-B", path, "-b", str(tmp_path / "j.bed"), "-o", outs[tag], "--flagstat", "--keepReads", "--minMapQ", "1"]) == 0
    proc.wait_deferred_close()
    from spliser_amd import flagstat as fstat, readstore
    plain = readstore.open_if_fresh(outs["plain"] + readstore.SUFFIX, sam, read_filter=(1, 0, 0))
    assert plain is not None and plain.n_reads > 5000
    for tag in ("bgzf", "gzip"):
        assert open(outs[tag] + ".SpliSER.tsv", "rb").read() == open(outs["plain"] + ".SpliSER.tsv", "rb").read(), tag
        assert open(outs[tag] + fstat.SUFFIX).read() == open(outs["plain"] + fstat.SUFFIX).read(), tag
        kept = readstore.open_if_fresh(outs[tag] + readstore.SUFFIX, str(tmp_path / ("b.sam.gz" if tag == "bgzf" else "g.sam.gz")), read_filter=(1, 0, 0))
        assert kept is not None and kept.n_reads == plain.n_reads, tag
        for name in case.ref_names:
            a, b = kept.reads(name), plain.reads(name)
            for k in ("pos", "flag", "cig_off", "cigar"):
                assert np.array_equal(getattr(a, k), getattr(b, k)), (tag, name, k)
