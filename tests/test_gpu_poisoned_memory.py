"""The device paths on poisoned and on reused device memory (poisoncases.py has the case list and the driver).

Every device buffer of the library comes from the pool of ``spl_capi.cpp``, which hands out dirty memory on purpose; every other
suite runs where memory nobody wrote reads as zero, so a read of scratch that nobody wrote passes there.  Here the list runs in two
fresh child processes, one after the other: the first with ``SPL_DEV_POISON=1`` -- every buffer is 0xA5 when it is handed out --,
the second without it and ``--twice``, forward and then in reverse order, so that the second pass meets buffers that hold the
first's plausible data (old hash keys, old boundaries, old mate indexes).  The children compute no expectation: what they left is
compared here with the yardsticks of the single suites, exactly.  A child that does not end with exit status 0 fails the fixture
with the tail of its output and of ``progress.log``, which names the case; the second child is then not started, and nothing is
run again.

The list covers the counting pass, the decodes, SAM text, every consumer of a finished set -- per read and per fragment --, the
junction table, the genome on the device (three window sizes on one set of buffers; a store that grows under joined sequences), the
motif kernel's strand bytes and tally, text, compressed text and FASTA in windows of 4096 bytes, two shards on two lanes, and the
commands end to end; poisoncases.py says what each case is there for.

Positive controls keep either mode from passing without having happened: the poisoned child's pool says that every buffer was
poisoned and a probe of 3 MiB + 1 bytes comes back as 4 MiB of 0xA5, a second one -- served from the pool -- again; the other
child's pool poisoned nothing and served more buffers from what it held during the second pass than before it."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import poisoncases as P
from spliser_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("poison", "reuse-first", "reuse-second")
CHILD_TIMEOUT = 300          # a safety cap, the one test_the_command_line_as_a_child_process uses; not a measurement


def _tail(text, n=40):
    return "\n".join(text.splitlines()[-n:])


def _child(out, poison, twice):
    """The driver in a fresh interpreter: -> (seconds, pool.json).  Fails with what the child said and where it was."""
    env = dict(os.environ)
    env.pop("SPL_DEV_POISON", None)
    if poison:
        env["SPL_DEV_POISON"] = "1"
    argv = [sys.executable, os.path.join(ROOT, "tests", "poisoncases.py"), "--out", out] + (["--twice"] if twice else [])
    t0 = time.time()
    try:
        r = subprocess.run(argv, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=CHILD_TIMEOUT)
        status, said = r.returncode, r.stdout
    except subprocess.TimeoutExpired as e:
        status, said = "none after %d s" % CHILD_TIMEOUT, e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode("utf-8", "replace")
    if status != 0:
        log = os.path.join(out, "progress.log")
        progress = open(log).read() if os.path.exists(log) else "(no progress.log)"
        pytest.fail("the %s child ended with exit status %s\n---- its output ----\n%s\n---- progress.log ----\n%s"
                    % ("poisoned" if poison else "unpoisoned", status, _tail(said), _tail(progress, 6)), pytrace=False)
    with open(os.path.join(out, "pool.json")) as fh:
        return time.time() - t0, json.load(fh)


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    native.build()
    d = tmp_path_factory.mktemp("poisoned")
    poison, reuse = str(d / "poison"), str(d / "reuse")
    out = {}
    out["poison_s"], out["poison_pool"] = _child(poison, True, False)
    out["reuse_s"], out["reuse_pool"] = _child(reuse, False, True)          # (not started when the first did not end well)
    out["dirs"] = {"poison": poison, "reuse-first": reuse, "reuse-second": os.path.join(reuse, "second")}
    print("\npoisoned child: %.1f s, pool %s\nunpoisoned child, twice: %.1f s, pool after the first pass %s, after the second %s"
          % (out["poison_s"], out["poison_pool"]["after_first_pass"], out["reuse_s"], out["reuse_pool"]["after_first_pass"], out["reuse_pool"]["after_second_pass"]))
    return out


@pytest.mark.parametrize("name", P.NAMES)
@pytest.mark.parametrize("mode", MODES)
def test_case(children, mode, name):
    got = P.load(os.path.join(children["dirs"][mode], name + ".npz"))
    bad = P.mismatches(got, P.want_of(name))
    assert not bad, "%s, %s:\n%s" % (name, mode, "\n".join(bad[:20]))


def test_the_poisoned_child_was_poisoned(children):
    pool = children["poison_pool"]
    stats = pool["after_first_pass"]
    assert stats["handed_out"] > 0 and stats["poisoned"] == stats["handed_out"]
    assert pool["probe_capacities"] == [4 << 20, 4 << 20]
    with np.load(os.path.join(children["dirs"]["poison"], "probes.npz")) as z:
        first, second = z["first"], z["second"]
    assert first.shape == second.shape == (4 << 20,)
    assert int(first.min()) == int(first.max()) == 0xA5
    # the second probe got a buffer the pool held (the first one's, given back), and it was poisoned again
    assert pool["after_second_probe"]["from_pool"] == pool["after_first_probe"]["from_pool"] + 1
    assert pool["after_second_probe"]["handed_out"] == pool["after_first_probe"]["handed_out"] + 1 == pool["after_second_probe"]["poisoned"]
    assert int(second.min()) == int(second.max()) == 0xA5


def test_the_unpoisoned_child_met_reused_buffers(children):
    pool = children["reuse_pool"]
    first, second = pool["after_first_pass"], pool["after_second_pass"]
    assert first["poisoned"] == second["poisoned"] == pool["after_second_probe"]["poisoned"] == 0
    handed, served = second["handed_out"] - first["handed_out"], second["from_pool"] - first["from_pool"]
    assert handed > 0 and served > 0          # the number served from the pool grew during the second pass
    print("\nsecond pass: %d of %d buffers came from the pool (%.1f %%); the pool holds %d bytes" % (served, handed, 100.0 * served / handed, second["held_bytes"]))


@pytest.mark.parametrize("child", ["poison_pool", "reuse_pool"])
def test_the_pool_hands_out_whole_granules_and_at_most_twice_what_was_asked(children, child):
    """A request is rounded up to the pool's 2 MiB granule and served by the smallest held buffer of at least that and at most twice
    that, or by a new one of exactly that: whatever the pool held after the list, the capacity lies between the two."""
    gran = 2 << 20
    asked = children[child]["capacities_by_request"]
    assert [b for b, _ in asked] == list(P.PROBE_SIZES)
    for b, cap in asked:
        want = (max(b, 1) + gran - 1) // gran * gran
        assert want <= cap <= 2 * want and cap % gran == 0, (b, cap)
