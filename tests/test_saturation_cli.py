"""The command line's refusals for ``saturation`` and ``junctions --subsample``, and the thresholds of the steps: no GPU, no file is
opened before the arguments are held to their ranges."""
import pytest

import subsamplecases as S
from spliser_amd import cli, readsets, saturation


def _refused(argv, capsys, what):
    with pytest.raises(SystemExit) as err:
        cli.main(argv)
    assert err.value.code == 2
    assert what in capsys.readouterr().err


BASE = ["saturation", "-B", "/nonexistent/x.bam", "-o", "/nonexistent/out"]


@pytest.mark.parametrize("extra, what", [(["--steps", "0"], "--steps must be in 1..100"), (["--steps", "101"], "--steps must be in 1..100"), (["-r", "0"], "must be at least 1"),
                                         (["-s", "auto"], "-s auto is not taken here"), (["--isStranded", "-s", "auto"], "-s auto is not taken here"),
                                         (["--isStranded"], "--isStranded requires"), (["--seed", "-1"], "--seed must be in"), (["--minMapQ", "256"], "--minMapQ must be in 0..255"),
                                         (["--minIntron", "-5"], "must not be negative")])
def test_saturation_refuses(extra, what, capsys):
    _refused(BASE + extra, capsys, what)


@pytest.mark.parametrize("extra, what", [(["--subsample", "0"], "fraction in (0, 1]"), (["--subsample", "1.5"], "fraction in (0, 1]"), (["--subsample", "-0.1"], "fraction in (0, 1]"),
                                         (["--seed", "4"], "--seed belongs to --subsample"), (["--subsample", "0.5", "--seed", "-2"], "--seed must be in")])
def test_junctions_subsample_refuses(extra, what, capsys):
    _refused(["junctions", "-B", "/nonexistent/x.bam", "-o", "/nonexistent/out.bed"] + extra, capsys, what)


def test_the_functions_refuse_what_the_command_line_refuses():
    for kwargs in (dict(steps=0), dict(steps=101), dict(minReads=0), dict(strandedType="auto")):
        with pytest.raises(ValueError):
            saturation.saturation("/nonexistent/x.bam", "/nonexistent/out", **kwargs)
    for f in (0, -1, 1.0001):
        with pytest.raises(ValueError):
            readsets.subsample_threshold(f)


def test_without_the_switches_junctions_arguments_are_what_they_were():
    args = vars(cli.build_parser(fragment_switches=True).parse_args(["junctions", "-B", "x", "-o", "y"]))
    assert "subsample" not in args and "seed" not in args
    args = vars(cli.build_parser(fragment_switches=True).parse_args(["junctions", "-B", "x", "-o", "y", "--subsample", "0.25", "--seed", "9"]))
    assert args["subsample"] == 0.25 and args["seed"] == 9


def test_thresholds_and_fractions():
    assert saturation.thresholds(4) == S.thresholds(4) == [2 ** 30, 2 ** 31, 3 * 2 ** 30, 2 ** 32]
    assert saturation.thresholds(20) == [(k << 32) // 20 for k in range(1, 21)] and saturation.thresholds(1) == [2 ** 32]
    assert readsets.subsample_threshold(0.5) == 2 ** 31 and readsets.subsample_threshold(1) == 2 ** 32 and readsets.subsample_threshold(1e-12) == 0
    assert saturation.HEADER.split() == ["step", "fraction", "reads", "junctions", "junctions_minReads", "junction_reads", "sites", "sites_minReads"]
