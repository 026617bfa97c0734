"""``csrc/spl_lanes.h`` alone in a program of its own under AddressSanitizer and UBSan (tests/hostsim/lanes_rule_asan.cpp): the
sequences of ``lanecases.py`` and seeded random ones, against the restatement."""
import os
import subprocess

import lanecases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE = 6 + 4 * 12


def test_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "lanes_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostsim", "lanes_rule_asan.cpp"), "-o", exe])
    cases = [(cfg, calls) for calls in list(L.SEQUENCES.values()) + [L.random_calls(s) for s in range(300)] + [[]]
             for cfg in ((1, 1, 0), (1, 1, 1), (0, 1, 0), (0, 0, 0))]
    lines = ["%d %d %d 64 64 | %s" % (cfg + (" ".join(str(v) for c in calls for v in c),)) for cfg, calls in cases]
    lines.append("1 1 0 1 1 | 1 5 0 1")                           # a table out of range
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stderr
    got = out.stdout.split("\n")
    assert len(got) >= len(lines) and got[len(cases)] == "error"
    for (cfg, calls), text in zip(cases, got):
        v = [int(x) for x in text.split()]
        assert len(v) == STRIDE * len(calls)
        plan = [dict(lane=r[0], piped=r[1], n_after=r[3], n_mid=r[4], tail_stream=r[5], ops=[tuple(r[6 + 4 * k:10 + 4 * k]) for k in range(r[2])])
                for r in (v[i:i + STRIDE] for i in range(0, len(v), STRIDE))]
        assert plan == L.restated_plan(calls, *cfg)
