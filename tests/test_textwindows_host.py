"""The window plan of the device's text sources on the host, no GPU: ``spl_text_windows_host`` (spliser_amd/csrc/spl_text_windows.h as
SamDecode and GenomeLoad call it) against the restatement of tests/windowcases.py under both long-line rules, on the smallest texts
at which a cut can go wrong and on random ones; the properties every plan has; and the header alone in a program under
AddressSanitizer and UBSan (tests/hostsim/text_windows_asan.cpp), every text in a heap block of exactly its size."""
import os
import subprocess

import pytest

import motifcases as M
import windowcases as Wc
from spliser_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = Wc.cases()
RULES = [(Wc.STOP, "stop"), (Wc.OWN, "own_window")]


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


def test_the_rules_are_the_librarys():
    assert (Wc.STOP, Wc.OWN) == (native.TEXT_WINDOWS_STOP, native.TEXT_WINDOWS_OWN)


def test_the_cases_have_what_they_are_for():
    plans = {(name, rule): Wc.window_plan(text, begin, window, rule) for name, text, begin, window in CASES for rule, _ in RULES}
    assert plans[("empty_body", Wc.STOP)] == ([], False) and plans[("empty_body", Wc.OWN)] == ([], False)
    assert plans[("begin_inside", Wc.STOP)][0][0] == (25, 25 + 60)
    for name in ("no_newline_shorter", "no_newline_equal", "window_larger_than_the_text"):
        assert len(plans[(name, Wc.STOP)][0]) == 1 and not plans[(name, Wc.STOP)][1], name
    assert plans[("no_newline_longer", Wc.STOP)] == ([], True) and plans[("no_newline_longer", Wc.OWN)] == ([(0, 65)], False)
    assert plans[("newline_is_the_windows_last_byte", Wc.STOP)][0][0] == (0, 64) and plans[("newline_is_the_first_byte_behind", Wc.STOP)][0][0] == (0, 11)
    assert plans[("line_of_a_window", Wc.STOP)][0][0] == (0, 64) and plans[("line_of_a_window_and_a_byte", Wc.STOP)] == ([], True)
    assert plans[("line_of_a_window_and_a_byte", Wc.OWN)][0][0] == (0, 65)
    assert plans[("crlf_cut_between", Wc.OWN)][0][:2] == [(0, 12), (12, 65)] and plans[("crlf_ends_a_window", Wc.OWN)][0][0] == (0, 64)
    stopped = {name for (name, rule), (_, long_line) in plans.items() if long_line}
    assert stopped >= {"long_first", "long_in_the_middle", "long_last_with_newline", "long_last_without_newline", "two_long_in_a_row", "header_only_then_long"}
    assert len(plans[("long_in_the_middle", Wc.STOP)][0]) == 2 and plans[("long_first", Wc.STOP)][0] == []
    own = plans[("two_long_in_a_row", Wc.OWN)][0]
    assert [hi - lo for lo, hi in own] == [40, 94, 192, 40]
    assert plans[("long_last_without_newline", Wc.OWN)][0][-1] == (80, 80 + 93) and plans[("long_last_with_newline", Wc.OWN)][0][-1] == (80, 80 + 94)


@pytest.mark.parametrize("rule,rule_name", RULES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_the_plan_is_the_restatement(built, case, rule, rule_name):
    name, text, begin, window = case
    want = Wc.window_plan(text, begin, window, rule)
    got = native.text_windows_host(text, begin, window, rule)
    assert got == want
    Wc.check_plan(text, begin, window, rule, *got)
    if rule == Wc.OWN and begin == 0:
        assert [hi for _, hi in got[0] if hi < len(text)] == M.window_cuts(text, window)


def test_random_texts(built):
    n_stopped = n_own = 0
    for name, text, begin, window in Wc.random_cases():
        for rule, _ in RULES:
            want = Wc.window_plan(text, begin, window, rule)
            got = native.text_windows_host(text, begin, window, rule)
            assert got == want, (name, rule)
            Wc.check_plan(text, begin, window, rule, *got)
            n_stopped += got[1]
            n_own += any(hi - lo > window for lo, hi in got[0])
        if begin == 0:
            assert [hi for _, hi in got[0] if hi < len(text)] == M.window_cuts(text, window), name
    assert n_stopped >= 50 and n_own >= 50          # (both rules met their long lines)


def test_the_pack_corpus_is_cut_as_its_own_restatement_says(built):
    text = M.pack_corpus()
    for window in (65536, 4096, 256 << 20):
        plan, long_line = native.text_windows_host(text, 0, window, Wc.OWN)
        assert not long_line and [hi for _, hi in plan if hi < len(text)] == M.window_cuts(text, window)
    assert native.text_windows_host(text, 0, 4096, Wc.STOP)[1]          # (its 40 000-base line fits no such window)


def test_bad_arguments_are_refused(built):
    for args in ((b"AA\n", 4, 64, 0), (b"AA\n", -1, 64, 0), (b"AA\n", 0, -1, 0), (b"AA\n", 0, 64, 2)):
        with pytest.raises(native.SpliserNativeError) as err:
            native.text_windows_host(*args)
        assert err.value.code == -1


def test_the_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "text_windows_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostsim", "text_windows_asan.cpp"), "-o", exe])
    lines, want = [], []
    for name, text, begin, window in CASES + Wc.random_cases():
        for rule, _ in RULES:
            lines.append("%d|%d|%d|%s" % (rule, begin, window, text.hex()))
            plan, long_line = Wc.window_plan(text, begin, window, rule)
            want.append(" ".join([str(int(long_line)), str(len(plan))] + ["%d %d" % w for w in plan]))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    done = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert done.returncode == 0, done.stderr[-3000:]
    got = done.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, lines[k][:80], g[:200], w[:200])
