"""``--genome`` / ``--strandFromMotif`` / ``--canonicalOnly`` on the device, against the restatement of tests/motifcases.py: the FASTA
packed on the GPU (``spl_genome_open``; default windows and windows of 64 KiB), the reads' strand bytes and the tally
(``spl_reads_motif_strand``) and a junction table's codes (``spl_junction_motifs``) on hand-built and random fused sets, and the two
commands end to end against the path that exists: ``--strandFromXS`` on the same reads carrying the tags the rule gives them."""
import numpy as np
import pytest

import motifcases as M
from spliser_amd import cli, native, samio

pytestmark = pytest.mark.gpu

XS3 = native.STRAND_FROM_XS


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


# ---- the pack ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    text = M.pack_corpus()
    path = tmp_path_factory.mktemp("fa") / "corpus.fa"
    path.write_bytes(text)
    return str(path), text, M.parse_fasta(text)


@pytest.mark.parametrize("window", [0, 65536])
def test_the_packed_genome_is_the_restatement(ctx, corpus, window):
    """(That windows of 64 KiB join sequences of this corpus inside a word of the store is asserted in tests/test_motif_host.py.)"""
    path, text, want = corpus
    with native.Genome(ctx, path, window) as g:
        assert g.names == [n.decode() for n, _ in want] and g.lengths == [len(c) for _, c in want]
        for k, (name, codes) in enumerate(want):
            assert np.array_equal(g.bases(k), codes), name
        k = g.names.index("long_line")
        assert np.array_equal(g.bases(k, 31, 70), want[k][1][31:101]) and g.bases(k, 40000, 0).size == 0
        stats = g.stats()
        assert stats["text_bytes"] == len(text) and stats["device_bytes"] == sum(16 * ((len(c) + 31) // 32) for _, c in want)
        assert stats["upload_ms"] > 0 and stats["pack_ms"] > 0
        with pytest.raises(native.SpliserNativeError):
            g.bases(0, 0, g.lengths[0] + 1)


def test_a_window_smaller_than_a_line(ctx, tmp_path):
    """Windows of 1 KiB under lines of 40 001 bases: such a line gets a window of its own, and the sequence is joined behind it, 1
    and 2 bases into a word of the store."""
    rng = np.random.default_rng(2)
    text = M.fasta_text([(b"a", M.random_bases(rng, 120004)), (b"b", M.random_bases(rng, 100))], width=40001)
    text += b"".join(b">s%d\n%s\n" % (k, M.random_bases(rng, 1 + k % 3)) for k in range(300))
    path = tmp_path / "long.fa"
    path.write_bytes(text)
    want = M.parse_fasta(text)
    assert [n % 32 for _, n in M.sequences_joined_across(text, 1024)[:4]] == [0, 1, 2, 3]
    with native.Genome(ctx, str(path), 1024) as g:
        assert g.names == [n.decode() for n, _ in want]
        assert all(np.array_equal(g.bases(k), c) for k, (_, c) in enumerate(want))


@pytest.mark.parametrize("window", [0, 65536])
def test_the_store_grows_under_many_short_sequences(ctx, tmp_path, window):
    """300 000 sequences of one or two bases under names of at most four letters: 16 bytes of store each, 4.8 MB, where the store is
    first given half the file's 2.4 MB -- more than twice that and 2 MiB, so no rounding of the first allocation holds it.  The
    store grows (window after window, with 64 KiB windows) and what the windows before stored is still there."""
    rng = np.random.default_rng(4)
    n = 300000
    names = [np.base_repr(k, 36).lower() for k in range(n)]
    bases = M.random_bases(rng, 2 * n)
    length = [2 if k % 31 == 0 else 1 for k in range(n)]
    text = "".join(">%s\n%s\n" % (names[k], bases[2 * k:2 * k + length[k]].decode()) for k in range(n)).encode()
    path = tmp_path / "short.fa"
    path.write_bytes(text)
    assert 16 * n > 2 * (len(text) // 2 + 4096) + (2 << 20)
    with native.Genome(ctx, str(path), window) as g:
        assert g.names == names and g.lengths == length
        assert g.stats()["device_bytes"] == 16 * n
        for k in list(range(0, 64)) + list(range(64, n, 997)) + [n - 1]:
            assert np.array_equal(g.bases(k), M.codes_of(bases[2 * k:2 * k + length[k]])), k


@pytest.mark.parametrize("case", range(len(M.format_errors())))
@pytest.mark.parametrize("window", [0, 65536])
def test_format_errors_name_the_line(ctx, tmp_path, case, window):
    text, line, why = M.format_errors()[case]
    path = tmp_path / "bad.fa"
    path.write_bytes(text)
    with pytest.raises(native.SpliserNativeError, match="line %d: .*%s" % (line, why)) as err:
        native.Genome(ctx, str(path), window)
    assert err.value.code == -5


def test_compressed_and_missing_files(ctx, tmp_path):
    import gzip
    path = tmp_path / "g.fa.gz"
    with gzip.open(str(path), "wb") as fh:
        fh.write(b">a\nACGT\n")
    with pytest.raises(native.SpliserNativeError, match="uncompressed FASTA") as err:
        native.Genome(ctx, str(path))
    assert err.value.code == -5
    with pytest.raises(native.SpliserNativeError) as err:
        native.Genome(ctx, str(tmp_path / "none.fa"))
    assert err.value.code == -4


# ---- the motif kernel --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def motif_cases(tmp_path_factory, ctx):
    """One FASTA with the planted and the random sequence (and one of no bases between them), on the device once; the restatement's
    answers computed once."""
    d = tmp_path_factory.mktemp("motif")
    planted, random = M.planted_case(), M.random_case(20261021, 5000)
    path = d / "two.fa"
    path.write_bytes(M.fasta_text([(b"planted", planted[0]), (b"none", b""), (b"random", random[0])], width=61))
    cases = {}
    for name, (bases, rs, juncs) in (("planted", planted), ("random", random)):
        seq = M.codes_of(bases)
        cases[name] = (seq, rs, juncs, M.expected(rs, seq))
    with native.Genome(ctx, str(path)) as g:
        yield g, cases


ELIGIBLE_OFF = 0x4 | 0x100 | 0x200 | 0x800


def _strands(ctx, genome, seq, rs, shift=0):
    """A fused set of the reads, every strand byte wrong before the call ('-') -> (tally, the mode-3 junction table, the reads that
    have a '+' or '-' byte afterwards among those ``spl_strand_tally`` looks at).  The table shows the byte of every read that has a
    junction, the count that every other read's byte is 0."""
    arrays = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, xs=np.full(rs.n, 45, np.uint8))
    with ctx.upload_soa([arrays], with_strand=True) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0, shift)
            dr.finish()
            assert dr.has_strand()
            assert int(dr.strand_tally()[2:8].sum()) == int(((rs.flag & ELIGIBLE_OFF) == 0).sum())      # (every byte is '-': all of them are tagged)
            tally = dr.motif_strand(genome, seq)
            assert dr.layout_bytes()[1] == 0 and dr.has_strand()          # (the set stays fused)
            return tally, dr.junctions(XS3, 0, 0, 0), int(dr.strand_tally()[2:8].sum())


@pytest.mark.parametrize("name", ["planted", "random"])
def test_strand_bytes_and_tally_are_the_restatement(ctx, motif_cases, name):
    genome, cases = motif_cases
    seq, rs, juncs, (want, want_tally) = cases[name]
    if name == "random":
        assert min(int((want == 43).sum()), int((want == 45).sum()), int(want_tally[9]), int(want_tally[10])) >= 100, want_tally
    tally, table, tagged = _strands(ctx, genome, name, rs)
    assert tally.tolist() == want_tally.tolist()
    got = {(int(l), int(r), int(s)): int(c) for l, r, s, c in zip(table["left"], table["right"], table["strand"], table["count"])}
    assert got == M.table_by_strand(rs, want)
    assert tagged == int(((want != 0) & ((rs.flag & ELIGIBLE_OFF) == 0)).sum())
    # ... and with the reads moved by a shift
    arrays = native.ReadArrays(rs.pos - 700, rs.flag, rs.cig_off, rs.cigar, xs=np.full(rs.n, 43, np.uint8))
    with ctx.upload_soa([arrays], with_strand=True) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0, 700)
            dr.finish()
            assert dr.motif_strand(genome, genome.index(name)).tolist() == want_tally.tolist()
            assert dr.layout_bytes()[1] == 0


def test_the_bytes_themselves_come_back(ctx, motif_cases):
    """A set whose bytes went up right gives the table the kernel's bytes give, row for row and column for column."""
    genome, cases = motif_cases
    seq, rs, _, _ = cases["random"]
    want = M.expected(rs, seq)[0]
    arrays = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, xs=want)
    with ctx.upload_soa([arrays], with_strand=True) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            by_upload = dr.junctions(XS3, 0, 0, 0)
    _, by_kernel, _ = _strands(ctx, genome, "random", rs)
    for k in by_upload:
        assert np.array_equal(by_upload[k], by_kernel[k]), k
    assert {43, 45, 63} == set(by_kernel["strand"].tolist())


def test_a_sequence_of_no_bases_and_sets_the_call_refuses(ctx, motif_cases):
    genome, cases = motif_cases
    seq, rs, _, _ = cases["planted"]
    tally, _, _ = _strands(ctx, genome, "none", samio.ReadSet.from_records([(0, 10, "5M50N5M"), (0, 20, "30M")]))
    assert tally.tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1]
    arrays = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)
    with ctx.upload_soa([arrays]) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            with pytest.raises(native.SpliserNativeError, match="strand bytes") as err:
                dr.motif_strand(genome, "planted")
            assert err.value.code == -1
    dr = ctx.upload_reads(arrays)
    try:
        with pytest.raises(native.SpliserNativeError, match="fused") as err:
            dr.motif_strand(genome, "planted")
        assert err.value.code == -1
    finally:
        dr.free()


@pytest.mark.parametrize("name", ["planted", "random"])
def test_junction_motifs_of_a_table(ctx, motif_cases, name):
    genome, cases = motif_cases
    seq, rs, juncs, _ = cases[name]
    extra = [(-5, 40), (-1, 30), (len(seq) - 10, len(seq) + 1), (len(seq), len(seq) + 50), (10, 12), (2147483000, 2147483600)]
    rows = juncs + extra
    got = genome.junction_motifs(name, [l for l, _ in rows], [r for _, r in rows])
    assert got.tolist() == [M.motif_code(seq, l, r)[0] for l, r in rows]
    assert genome.junction_motifs(name, [], []).size == 0


# ---- end to end, against the path that exists -------------------------------------------------------------------------------------
NAMES = ["c1", "c2", "c3"]


@pytest.fixture(scope="module")
def command_files(tmp_path_factory):
    """Three chromosomes: the reads without tags (BAM and SAM text), the same reads with the XS:A tags the rule gives them, the FASTA
    -- in another order than the header's, with a sequence nobody aligned to --, and one whose c2 is a base short."""
    d = str(tmp_path_factory.mktemp("cmd"))
    made = [M.random_case(100 + k, 1200) for k in range(3)]
    sets = [(c, rs) for c, (_, rs, _) in zip(NAMES, made)]
    bases = {c: b for c, (b, _, _) in zip(NAMES, made)}
    seqs = {c: M.codes_of(b) for c, b in bases.items()}
    lengths = [len(bases[c]) for c in NAMES]
    tags = [M.expected_xs_tags(rs, seqs[c]) for c, rs in sets]
    samio.write_bam(d + "/plain.bam", NAMES, lengths, sets, with_seq=True)
    samio.write_bam(d + "/tagged.bam", NAMES, lengths, sets, with_seq=True, tags=tags)
    for name, with_tags in (("plain.sam", False), ("tagged.sam", True)):
        with open(d + "/" + name, "w") as fh:
            fh.write("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in zip(NAMES, lengths)))
            for (chrom, rs), tg in zip(sets, tags):
                for k in range(rs.n):
                    cols = ["r", str(rs.flag[k]), chrom, str(rs.pos[k]), "60", samio.cigar_string(rs.cigar[rs.cig_off[k]:rs.cig_off[k + 1]]), "*", "0", "0", "*", "*"]
                    fh.write("\t".join(cols + (["XS:A:" + tg[k][3:].decode()] if with_tags and tg[k] else [])) + "\n")
    order = [("c3", bases["c3"]), ("extra", b"ACGTNNNN" * 40), ("c1", bases["c1"]), ("c2", bases["c2"])]
    with open(d + "/g.fa", "wb") as fh:
        fh.write(M.fasta_text([(n.encode(), b) for n, b in order], width=70))
    with open(d + "/short.fa", "wb") as fh:
        fh.write(M.fasta_text([(n.encode(), b[:-1] if n == "c2" else b) for n, b in order], width=70))
    with open(d + "/missing.fa", "wb") as fh:
        fh.write(M.fasta_text([(n.encode(), b) for n, b in order if n != "c3"], width=70))
    return d, sets, seqs


@pytest.mark.parametrize("tag,ext,pflags", [("device", "bam", []), ("host", "bam", ["--hostDecode"]), ("shares", "bam", ["--devices", "0,0"]),
                                            ("sam", "sam", [])])
def test_motif_strands_write_what_the_tags_write(tag, ext, pflags, command_files, capsys):
    d, sets, seqs = command_files
    plain, tagged, fa = "%s/plain.%s" % (d, ext), "%s/tagged.%s" % (d, ext), d + "/g.fa"
    by_motif, by_tag = "%s/%s.motif" % (d, tag), "%s/%s.tag" % (d, tag)
    if not pflags:
        assert cli.main(["junctions", "-B", plain, "-o", by_motif + ".bed", "--genome", fa, "--strandFromMotif"]) == 0
        log = capsys.readouterr().out
        assert "strand from motif: reads +:" in log and "GT/AG:" in log
        want = sum(M.expected(rs, seqs[c])[1] for c, rs in sets)
        assert "reads +: %d, -: %d, conflicting: %d, spliced without a canonical motif: %d;" % tuple(want[7:11]) in log
        assert cli.main(["junctions", "-B", tagged, "-o", by_tag + ".bed", "--strandFromXS"]) == 0
        text = open(by_motif + ".bed").read()
        assert text == open(by_tag + ".bed").read()
        assert {line.split("\t")[5] for line in text.splitlines()[1:]} == {"+", "-", "?"}
    assert cli.main(["process", "-B", plain, "-o", by_motif, "--genome", fa, "--strandFromMotif", "--keepJunctions"] + pflags) == 0
    assert cli.main(["process", "-B", tagged, "-o", by_tag, "--strandFromXS", "--keepJunctions"] + pflags) == 0
    got = open(by_motif + ".SpliSER.tsv").read()
    assert got == open(by_tag + ".SpliSER.tsv").read() and got.count("\n") > 50
    assert open(by_motif + ".junctions.bed").read() == open(by_tag + ".junctions.bed").read()
    assert {"+", "-"} <= {line.split("\t")[2] for line in got.splitlines()[1:]}


def _bed_rows(path):
    lines = open(path).read().splitlines()
    rows = []
    for line in lines[1:]:
        c = line.split("\t")
        sizes = c[10].split(",")
        rows.append((c, int(c[1]) + int(sizes[0]), int(c[2]) - int(sizes[1])))
    return lines[0], rows


@pytest.mark.parametrize("strand_flags", [[], ["--strandFromMotif"]])
def test_canonical_only_drops_the_rows_the_restatement_codes_0(strand_flags, command_files, capsys):
    d, sets, seqs = command_files
    plain, fa = d + "/plain.bam", d + "/g.fa"
    tag = "canon%d" % len(strand_flags)
    all_bed, kept_bed = "%s/%s.all.bed" % (d, tag), "%s/%s.kept.bed" % (d, tag)
    genome_flags = ["--genome", fa] + strand_flags
    assert cli.main(["junctions", "-B", plain, "-o", all_bed] + (genome_flags if strand_flags else [])) == 0
    capsys.readouterr()
    assert cli.main(["junctions", "-B", plain, "-o", kept_bed, "--canonicalOnly"] + genome_flags) == 0
    log = capsys.readouterr().out
    head, rows = _bed_rows(all_bed)
    want, dropped, dropped_reads = [head], 0, 0
    for cols, left, right in rows:
        if M.motif_code(seqs[cols[0]], left, right)[0] == 0:
            dropped, dropped_reads = dropped + 1, dropped_reads + int(cols[4])
            continue
        want.append("\t".join(cols[:3] + ["JUNC%08d" % len(want)] + cols[4:]))
    assert dropped >= 10 and len(want) > 30
    assert open(kept_bed).read() == "\n".join(want) + "\n"
    assert "dropped:\t%d (%d supporting reads)" % (dropped, dropped_reads) in log
    out = "%s/%s.process" % (d, tag)
    assert cli.main(["process", "-B", plain, "-o", out, "--canonicalOnly", "--keepJunctions"] + genome_flags) == 0
    assert open(out + ".junctions.bed").read() == open(kept_bed).read()
    assert cli.main(["process", "-B", plain, "-b", kept_bed, "-o", out + ".b"]) == 0
    assert open(out + ".SpliSER.tsv").read() == open(out + ".b.SpliSER.tsv").read()


def test_a_fasta_that_is_not_the_alignments_genome(command_files):
    d, _, seqs = command_files
    n = len(seqs["c2"])
    with pytest.raises(native.SpliserNativeError, match="c2 is %d in the alignment and %d in the FASTA: is this the genome the reads were aligned to" % (n, n - 1)):
        cli.main(["junctions", "-B", d + "/plain.bam", "-o", d + "/never.bed", "--genome", d + "/short.fa", "--strandFromMotif"])
    with pytest.raises(native.SpliserNativeError, match="c3 is in the alignment and not in the FASTA"):
        cli.main(["junctions", "-B", d + "/plain.bam", "-o", d + "/never.bed", "--genome", d + "/missing.fa", "--canonicalOnly"])
    # ... and a chromosome the command does not visit need not be there
    assert cli.main(["junctions", "-B", d + "/plain.bam", "-o", d + "/c1.bed", "--genome", d + "/missing.fa", "--strandFromMotif", "-c", "c1"]) == 0
