"""The motif rule on the host, no GPU: ``spl_genome_pack_host``, ``spl_motif_read_strand_host`` and ``spl_junction_motifs_host`` against
the restatement of tests/motifcases.py on the pack corpus, the hand-built reads and random reads; the rule header alone in a
program under AddressSanitizer and UBSan (tests/hostsim/motif_rule_asan.cpp) over hostile inputs; the command line's refusals."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import motifcases as M
from spliser_amd import cli, native, samio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


@pytest.fixture(scope="module")
def corpus():
    text = M.pack_corpus()
    return text, M.parse_fasta(text)


def _same_sequences(got, want):
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, a), (_, b) in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a, b), name


def test_the_corpus_has_what_it_is_for(corpus):
    text, seqs = corpus
    lengths = {n: len(c) for n, c in seqs}
    assert len(text) < 1000000 and len(seqs) >= 70 and not text.endswith(b"\n")
    assert [lengths[b"len%d" % n] for n in (0, 1, 31, 32, 33)] == [0, 1, 31, 32, 33]
    assert lengths[b"long_line"] == 40000 and lengths[b"one_base_lines"] == 97 and lengths[b"crlf"] == 463 and lengths[b"crlf_name_only"] == 5
    ends = [k for k in range(len(text)) if text[k:k + 1] == b"\n"]
    assert {(e + 1) % M.CHUNK for e in ends} >= {0, 1, M.CHUNK - 1}          # a line ends on a chunk edge, and one byte either side
    at = text.index(b">header_across")
    assert at // M.CHUNK != text.index(b"\n", at) // M.CHUNK
    assert any(0 in c for _, c in seqs) and lengths[b"last_without_newline"] == 62


def test_the_corpus_is_joined_across_windows_inside_a_store_word(corpus):
    """What windows of 64 KiB are for: sequences go on across a cut with a number of bases that is no multiple of 32, so the later
    window's first lane reads back the 16-byte word the earlier launch stored -- asserted of the corpus, on the CPU."""
    text, _ = corpus
    joined = M.sequences_joined_across(text, 65536)
    assert len(joined) >= 5 and sum(1 for _, n in joined if n % 32) >= 3, joined
    assert any(text[cut - 2:cut] == b"\r\n" for cut, _ in joined)          # ... one of them behind a CRLF pair
    assert M.sequences_joined_across(text, 256 << 20) == []


def test_pack_host_is_the_restatement(built, corpus):
    text, want = corpus
    _same_sequences(native.genome_pack_host(text), want)
    for text in (b">a\n", b">a", b">a\r\n\r\n>b x\nAC\r", b">a\nACGT", b">x\n\n\nAC\n\nGT\n"):      # no bases; no newline; a CR that is a base
        _same_sequences(native.genome_pack_host(text), M.parse_fasta(text))
    assert [len(c) for _, c in native.genome_pack_host(b">a\r\n\r\n>b x\nAC\r")] == [0, 3]


@pytest.mark.parametrize("text,line,why", M.format_errors() + [(gzip.compress(b">a\nAC\n", mtime=0), 1, "uncompressed FASTA")])     # (mtime: the case's id is its bytes, and must not change with the clock)
def test_pack_host_declines_with_the_line(built, text, line, why):
    with pytest.raises(M.FastaError) as want:
        M.parse_fasta(text)
    assert want.value.line == line
    with pytest.raises(native.SpliserNativeError, match="line %d: .*%s" % (line, why)) as err:
        native.genome_pack_host(text)
    assert err.value.code == -5


def _arrays(rs):
    return native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (bases, rs, juncs) in (("planted", M.planted_case()), ("random", M.random_case(5, 2000))):
        seq = M.codes_of(bases)
        out[name] = (seq, rs, juncs, M.expected(rs, seq))
    return out


@pytest.mark.parametrize("name", ["planted", "random"])
def test_read_strand_host_is_the_restatement(built, cases, name):
    seq, rs, juncs, (want, want_tally) = cases[name]
    got, tally = native.motif_read_strand_host(_arrays(rs), seq)
    assert np.array_equal(got, want) and tally.tolist() == want_tally.tolist()
    assert all(want_tally[1:11] > 0), want_tally                     # every motif is walked, every class of read is there
    left, right = np.array([j[0] for j in juncs]), np.array([j[1] for j in juncs])
    assert native.junction_motifs_host(seq, left, right).tolist() == [M.motif_code(seq, l, r)[0] for l, r in juncs]
    # a shift moves the reads, not the sequence
    moved = samio.ReadSet(rs.pos - 1000, rs.flag, rs.cig_off, rs.cigar)
    got, tally = native.motif_read_strand_host(_arrays(moved), seq, shift=1000)
    assert np.array_equal(got, want) and tally.tolist() == want_tally.tolist()


def test_the_planted_case_has_what_it_is_for(cases):
    seq, rs, juncs, (want, tally) = cases["planted"]
    codes = [M.motif_code(seq, l, r) for l, r in juncs]
    assert {c for c, _ in codes} == set(range(7)) and tally[11] >= 2 and tally[9] >= 3
    for code in range(1, 7):
        assert {l % 2 for (l, r), (c, _) in zip(juncs, codes) if c == code} == {0, 1}, code
    assert any(l % 32 == 31 and c for (l, r), (c, _) in zip(juncs, codes)) and any(r % 32 == 1 and c for (l, r), (c, _) in zip(juncs, codes))
    assert (0, 40) in juncs and (len(seq) - 50, len(seq)) in juncs
    assert [M.motif_code(seq, 8000 + 100 * k, 8000 + 101 * k)[0] for k in (1, 2, 3, 4, 5)] == [0, 0, 0, 1, 1]
    n_ops = np.diff(rs.cig_off.astype(np.int64))
    assert n_ops.max() == 141 and want[int(np.argmax(n_ops))] == 0 and 43 in want[n_ops == 139]      # 70 N ops: conflicting; 69: '+'


def test_the_rule_header_under_the_sanitizers(tmp_path, built, corpus, cases):
    exe = str(tmp_path / "motif_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostsim", "motif_rule_asan.cpp"), "-o", exe])
    text_of = lambda v: " ".join(str(int(x)) for x in v)
    lines, want = [], []

    def fasta_case(text):
        lines.append("F|" + bytes(text).hex())
        try:
            seqs = M.parse_fasta(text)
        except M.FastaError as exc:
            reason = {"bytes before the first header": 1, "empty name": 2, "repeated name": 3, "no sequence": 4, "gzip": 5}[exc.reason]
            want.append("E %d %d" % (reason, exc.line))
            return
        want.append("S %d" % len(seqs))
        want.extend(("%s %d %s" % (name.hex(), len(codes), codes.tobytes().hex())) for name, codes in seqs)

    def reads_case(seq, rs, shift=0, off=None, expect=None):
        lines.append("|".join(["R", str(shift), seq.tobytes().hex(), text_of(rs.pos), text_of(rs.flag), text_of(rs.cig_off if off is None else off), text_of(rs.cigar)]))
        got, tally = expect if expect is not None else M.expected(rs, seq, shift)
        want.extend([text_of(got), text_of(tally)])

    text, _ = corpus
    fasta_case(text)
    for bad, _, _ in M.format_errors()[:4]:
        fasta_case(bad)
    for text in (b"", b">", b">a", b">chr1 a header the file ends in", b">a\n", b">a\nAC\n>b", b">a\r", b"\r", b"\n", b">a\nA", b"\x1f\x8b\x08", b"\x1f", b">a\n\r\n\r"):
        fasta_case(text)
    for name in ("planted", "random"):
        seq, rs, juncs, _ = cases[name]
        reads_case(seq, rs)
        lines.append("|".join(["J", seq.tobytes().hex(), text_of([j[0] for j in juncs]), text_of([j[1] for j in juncs])]))
        want.append(text_of([M.motif_code(seq, l, r)[0] for l, r in juncs]))
    # hostile: junctions in front of base 1 and beyond the end, a sequence of no bases and of three, offsets beyond the ops and descending
    seq, rs, _, _ = cases["planted"]
    reads_case(seq, rs, shift=-5000)
    reads_case(seq, rs, shift=15000)
    reads_case(seq[:0], rs)
    reads_case(seq[:3], rs)
    far = samio.ReadSet.from_records([(0, 2147483000, "100M400N100M"), (0, 2147483500, "50M200N50M"), (0, 1, "2147483000N5M")])
    reads_case(seq, far)
    one = samio.ReadSet.from_records([(0, 101, "20M81N20M"), (0, 401, "20M81N20M")])
    good = M.expected(one, seq)[0]
    reads_case(seq, one, off=[0, 3, 9], expect=(np.array([good[0], 0]), M.expected(samio.ReadSet.from_records([(0, 101, "20M81N20M")]), seq)[1]))
    both = M.expected(samio.ReadSet.from_records([(0, 401, "20M81N20M20M81N20M")]), seq)       # (offsets that descend: no ops; then all six for the second read)
    reads_case(seq, one, off=[3, 0, 6], expect=(np.array([0, both[0][0]]), both[1]))
    lines.append("|".join(["J", seq.tobytes().hex(), "-100 -1 0 19990 19996 20000 5 -2147483648", "-50 40 3 20000 20001 20100 2147483647 2147483647"]))
    want.append(text_of([M.motif_code(seq, l, r)[0] for l, r in zip((-100, -1, 0, 19990, 19996, 20000, 5, -2147483648), (-50, 40, 3, 20000, 20001, 20100, 2147483647, 2147483647))]))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    done = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert done.returncode == 0, done.stderr[-3000:]
    got = done.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g[:200], w[:200])


# ---- the command line's refusals -------------------------------------------------------------------------------------------------
@pytest.fixture()
def fasta(tmp_path):
    path = tmp_path / "g.fa"
    path.write_bytes(b">c1\nACGT\n")
    return str(path)


def _refused(argv, capsys, *words):
    with pytest.raises(SystemExit) as err:
        cli.main(argv)
    assert err.value.code == 2
    message = capsys.readouterr().err
    for w in words:
        assert w in message, message


@pytest.mark.parametrize("command", ["junctions", "process"])
def test_alternatives_and_what_needs_the_genome(command, fasta, capsys, tmp_path):
    base = [command, "-B", "x.bam", "-o", str(tmp_path / "out")]
    _refused(base + ["--strandFromMotif"], capsys, "--strandFromMotif", "--genome")
    _refused(base + ["--canonicalOnly"], capsys, "--canonicalOnly", "--genome")
    _refused(base + ["--genome", fasta, "--strandFromMotif", "--strandFromXS"], capsys, "--strandFromMotif", "--strandFromXS")
    _refused(base + ["--genome", fasta, "--strandFromMotif", "--isStranded", "-s", "fr"], capsys, "--strandFromMotif", "--isStranded")
    _refused(base + ["--genome", fasta, "--strandFromMotif", "-s", "auto"], capsys, "--strandFromMotif", "-s auto")
    packed = str(tmp_path / "g.fa.gz")
    with gzip.open(packed, "wb") as fh:
        fh.write(b">c1\nACGT\n")
    _refused(base + ["--genome", packed, "--strandFromMotif"], capsys, "uncompressed FASTA")
    _refused(base + ["--genome", str(tmp_path / "none.fa")], capsys, "none.fa")


def test_the_genome_does_not_go_with_a_junction_file(fasta, capsys, tmp_path):
    base = ["process", "-B", "x.bam", "-b", "x.bed", "-o", str(tmp_path / "out"), "--genome", fasta]
    _refused(base, capsys, "--genome", "--bedFile")
    _refused(base + ["--strandFromMotif"], capsys, "--strandFromMotif", "--bedFile")
    _refused(base + ["--canonicalOnly"], capsys, "--canonicalOnly", "--bedFile")


def test_the_functions_refuse_what_the_command_line_refuses(fasta, tmp_path):
    from spliser_amd import junctions as jn, process as proc
    out = str(tmp_path / "o")
    for kw, words in ((dict(strandFromMotif=True), "needs genome"), (dict(canonicalOnly=True), "needs genome"),
                      (dict(genome=fasta, strandFromMotif=True, strandFromXS=True), "strandFromXS"),
                      (dict(genome=fasta, strandFromMotif=True, isStranded=True, strandedType="fr"), "isStranded"),
                      (dict(genome=fasta, strandFromMotif=True, strandedType="auto"), "auto")):
        with pytest.raises(ValueError, match=words):
            jn.junctions("x.bam", out, **kw)
        with pytest.raises(ValueError, match=words):
            proc.process("x.bam", None, out, **kw)
    with pytest.raises(ValueError, match="without inBed"):
        proc.process("x.bam", "x.bed", out, genome=fasta)
