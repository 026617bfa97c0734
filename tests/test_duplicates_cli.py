"""The command line of ``duplicates`` and ``--dedup``: the refusals, the help text, and that without the switch the parsed arguments
of ``junctions``, ``genecounts`` and ``saturation`` are what they were, key for key.  No GPU, no file is opened before the arguments
are held to their ranges."""
import pytest

import dupcases as D
from spliser_amd import cli, duplicates, native, readsets, saturation


def _refused(argv, capsys, what):
    with pytest.raises(SystemExit) as err:
        cli.main(argv)
    assert err.value.code == 2
    assert what in capsys.readouterr().err


BASE = ["duplicates", "-B", "/nonexistent/x.bam", "-o", "/nonexistent/out"]


@pytest.mark.parametrize("argv, what", [(["duplicates", "-B", "x.bam"], "-o/--outputPath"), (["duplicates", "-o", "out"], "-B/--BAMFile"),
                                        (BASE + ["--minMapQ", "256"], "--minMapQ must be in 0..255"), (BASE + ["--requireFlags", "0x400", "--excludeFlags", "0x400"], "share a bit"),
                                        (BASE + ["--dedup"], "unrecognized arguments"), (BASE + ["-A", "genes.gtf"], "unrecognized arguments")])
def test_duplicates_refuses(argv, what, capsys):
    _refused(argv, capsys, what)


@pytest.mark.parametrize("command", ["process", "coverage", "exoncounts", "intronretention", "strandedness", "flagstat"])
def test_dedup_belongs_to_three_commands(command, capsys):
    """``process --dedup`` and the others are out of scope: the switch is not theirs."""
    _refused([command, "-B", "/nonexistent/x.bam", "-o", "/nonexistent/out", "-A", "/nonexistent/a.gtf", "--dedup"], capsys, "--dedup")


def test_dedup_takes_no_value(capsys):
    _refused(["junctions", "-B", "/nonexistent/x.bam", "-o", "/nonexistent/out.bed", "--dedup", "yes"], capsys, "unrecognized arguments")
    _refused(["junctions", "-B", "/nonexistent/x.bam", "-o", "/nonexistent/out.bed", "--dedup", "--seed", "4"], capsys, "--seed belongs to --subsample")
    _refused(["saturation", "-B", "/nonexistent/x.bam", "-o", "/nonexistent/out", "--dedup", "-s", "auto"], capsys, "-s auto is not taken here")
    _refused(["genecounts", "-B", "/nonexistent/x.bam", "-o", "/nonexistent/out", "--dedup"], capsys, "--annotationFile/-A is required")


def _help(argv, capsys):
    with pytest.raises(SystemExit) as err:
        cli.build_parser(fragment_switches=True).parse_args(argv)
    assert err.value.code == 0
    return " ".join(capsys.readouterr().out.split())


def test_the_help_text(capsys):
    text = _help(["duplicates", "--help"], capsys)
    for word in (".duplicates.tsv", ".duplicates.hist.tsv", "--anyOrder", "--hostDecode", "--excludeFlags", "-c"):
        assert word in text, word
    for command in ("junctions", "genecounts", "saturation"):
        text = _help([command, "--help"], capsys)
        assert "--dedup" in text and "smallest name hash" in text and "`duplicates`" in text
    assert "fraction is chosen first" in _help(["junctions", "--help"], capsys)
    assert "reads_before_dedup" in _help(["saturation", "--help"], capsys)
    assert "duplicates" in _help(["--help"], capsys)


PARENT = {
    "junctions": (["junctions", "-B", "x", "-o", "y"],
                  {'command': 'junctions', 'inBAM': 'x', 'outputPath': 'y', 'qChrom': 'All', 'isStranded': False, 'strandedType': None, 'minEvidence': None, 'strandFromXS': False,
                   'genome': None, 'strandFromMotif': False, 'canonicalOnly': False, 'minAnchor': 8, 'minIntron': 70, 'maxIntron': 500000, 'anyOrder': False, 'minMapQ': 0,
                   'requireFlags': 0, 'excludeFlags': 0, 'gpus': 1, 'devices': None, 'threads': 0}),
    "genecounts": (["genecounts", "-B", "x", "-A", "a", "-o", "y"],
                   {'command': 'genecounts', 'inBAM': 'x', 'annotationFile': 'a', 'outputPath': 'y', 'aType': 'exon', 'idAttr': 'gene_id', 'qChrom': 'All', 'isStranded': False,
                    'strandedType': None, 'gpuDecode': None, 'anyOrder': False, 'fragments': False, 'minMapQ': 0, 'requireFlags': 0, 'excludeFlags': 0, 'gpus': 1,
                    'devices': None, 'threads': 0}),
    "saturation": (["saturation", "-B", "x", "-o", "y"],
                   {'command': 'saturation', 'inBAM': 'x', 'outputPath': 'y', 'steps': 20, 'seed': 0, 'minReads': 10, 'qChrom': 'All', 'isStranded': False, 'strandedType': None,
                    'minAnchor': 8, 'minIntron': 70, 'maxIntron': 500000, 'gpuDecode': None, 'anyOrder': False, 'minMapQ': 0, 'requireFlags': 0, 'excludeFlags': 0, 'gpus': 1,
                    'devices': None, 'threads': 0}),
}


@pytest.mark.parametrize("command", sorted(PARENT))
def test_without_the_switch_the_arguments_are_what_they_were(command):
    argv, want = PARENT[command]
    for switches in (True, False):
        assert vars(cli.build_parser(fragment_switches=switches).parse_args(argv)) == want
        assert vars(cli.build_parser(fragment_switches=switches).parse_args(argv + ["--dedup"])) == dict(want, dedup=True)


def test_the_arguments_of_duplicates():
    args = vars(cli.build_parser().parse_args(BASE + ["-c", "Chr2", "--anyOrder", "--hostDecode", "--excludeFlags", "0x900"]))
    assert args == dict(command="duplicates", inBAM="/nonexistent/x.bam", outputPath="/nonexistent/out", qChrom="Chr2", anyOrder=True, gpuDecode=False, minMapQ=0, requireFlags=0,
                        excludeFlags=0x900, gpus=1, devices=None, threads=0)


def test_the_tables_text():
    """The two files as the issue words them, by the module's own writers and by the restatement's."""
    assert duplicates.HEADER.split() == ["chrom", "reads", "examined", "pair_fragments", "single_fragments", "duplicate_pairs", "duplicate_singles", "duplicate_reads",
                                         "flagged_in_file", "fraction_duplicated"]
    assert duplicates.HIST_HEADER.split() == ["group_size", "groups"] and native.DUP_COUNTS == D.COUNTS
    assert duplicates.row_text("c", [10, 9, 3, 3, 1, 1, 2]) == "c\t10\t9\t3\t3\t1\t1\t3\t2\t%r\n" % (3 / 9)
    assert duplicates.row_text("c", [4, 0, 0, 0, 0, 0, 0]).endswith("\t0\t0\tNA\n")
    assert saturation.HEADER.split() == ["step", "fraction", "reads", "junctions", "junctions_minReads", "junction_reads", "sites", "sites_minReads"]


def test_the_source_a_dedup_needs():
    class Source(object):
        mate_keys, shares = False, None
    with pytest.raises(native.SpliserNativeError, match="name keys"):
        readsets.check_fragment_source(Source())
