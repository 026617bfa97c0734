"""``spl_reads_duplicates`` and ``spl_reads_dedup`` on the device against the restatement of ``dupcases.py``, exactly: the marks, the
seven counters and the histogram of every segment of every case, asked twice of one set and of a second set made afterwards; the
deduplicated set's arrays and index against numpy's mask through every consumer of a fused set (``dup_device.py``).  The refusals
are ``spl_mate_table``'s and leave the context usable.  The same cases once more in one fresh child process on poisoned device
memory (``SPL_DEV_POISON=1``)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dup_device as DD
import dupcases as D
import matecases as M
import subsample_device as V
from spliser_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300          # a safety cap, the one test_gpu_poisoned_memory.py gives its children; not a measurement


@pytest.fixture(scope="module")
def ctx():
    native.build()
    with native.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def tile():
    native.build()
    return native.subsample_tile()


@pytest.fixture(scope="module")
def wanted(ctx, tile):
    """Per case what the restatement and numpy say, computed once: the in-process tests and the child's results are held to it."""
    return {name: (segs, with_strand, DD.want_of(ctx, segs, with_strand)) for name, segs, with_strand in DD.case_list(tile)}


PARTS = 4


@pytest.mark.parametrize("part", range(PARTS))
def test_cases(ctx, wanted, part):
    """Every case, and behind it the same case on a second set made afterwards (the pool hands the first one's buffers out again)."""
    seen = 0
    for k, (name, (segs, with_strand, want)) in enumerate(wanted.items()):
        if k % PARTS != part:
            continue
        for turn in range(2):
            bad = V.mismatches(DD.got_of(ctx, segs, with_strand), want)
            assert not bad, "%s, turn %d:\n%s" % (name, turn, "\n".join(bad[:20]))
        seen += 1
    assert seen


def test_the_cases_are_the_issues(tile):
    cases = D.all_cases(tile)
    D.assert_covers(cases, tile)
    assert {"corners", "group_across_tiles", "group_255_and_256", "all_unique", "all_one_group", "empty_middle"} <= {n for n, _ in cases}
    assert native.DUP_COUNTS == D.COUNTS


def test_the_deduplicated_set_pairs_the_same_names(ctx, tile):
    rng = np.random.default_rng(31)
    rs = D.crowd(rng, 2 * tile + 3)
    dup = D.duplicates(rs, rs.keys.tolist())[0]
    assert dup.any()
    mate = np.array(M.mate_table_of(rs, rs.keys.tolist())[0], np.int64)
    with V.fused(ctx, [rs], False) as dr:
        sel, kept, index = dr.dedup(with_index=True)
        try:
            got, counts = sel.mate_table(0, int(kept[0]))
        finally:
            sel.free()
    assert np.array_equal(index, np.flatnonzero(~dup))
    back = np.full(rs.n, -1, np.int64)
    back[index] = np.arange(len(index))
    want = np.where(mate[index] == M.NONE, M.NONE, back[np.where(mate[index] == M.NONE, 0, mate[index])])          # (a kept read's mate is kept)
    assert np.array_equal(got.astype(np.int64), want) and counts["paired"] == int((want != M.NONE).sum())
    paired = np.flatnonzero(got != M.NONE)
    assert np.array_equal(rs.keys[index][paired] >> np.uint64(1), rs.keys[index][got[paired]] >> np.uint64(1))


def test_the_same_words_from_run_to_run(ctx, tile):
    rs = D.joined(D.one_group(np.random.default_rng(32), tile + 200, True), D.crowd(np.random.default_rng(33), tile))
    runs = []
    for _ in range(3):
        with V.fused(ctx, [rs], False) as dr:
            dup, counts, hist = dr.duplicates(0, rs.n)
            runs.append((dup.tobytes(), counts, hist.tobytes()))
    assert runs[0] == runs[1] == runs[2]
    assert runs[0][1] == D.duplicates(rs, rs.keys.tolist())[1]


def test_a_set_without_a_read(ctx):
    with ctx.begin_reads() as dr:
        dr.finish()
        dup, counts, hist = dr.duplicates(0, 0)
        assert not len(dup) and not any(counts.values()) and not hist.any()
        sel, kept = dr.dedup()
        try:
            assert sel.n == 0 and not len(kept)
        finally:
            sel.free()


def test_refusals_are_the_mate_tables_and_leave_the_context_usable(ctx):
    rs = D.crowd(np.random.default_rng(34), 9)
    plain = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)

    def fine():
        with V.fused(ctx, [rs], False) as dr:
            assert dr.duplicates(0)[1] == D.duplicates(rs, rs.keys.tolist())[1]
            sel, kept = dr.dedup()
            sel.free()

    with V.fused(ctx, [rs], False) as dr:
        for seg in (-1, 1):
            with pytest.raises(native.SpliserNativeError, match="no segment") as err:
                dr.duplicates(seg)
            assert err.value.code == -1
    fine()
    with ctx.upload_soa([plain]) as soa:          # no keys
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            for call in (lambda: dr.duplicates(0), dr.dedup):
                with pytest.raises(native.SpliserNativeError, match="name keys") as err:
                    call()
                assert err.value.code == -1
    fine()
    with ctx.upload_soa([V._arrays(rs, False)], with_keys=True) as soa:          # not finished
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            for call in (lambda: dr.duplicates(0), dr.dedup):
                with pytest.raises(native.SpliserNativeError, match="not finished") as err:
                    call()
                assert err.value.code == -1
    fine()
    dr = ctx.upload_reads(plain)          # packed on the host: records, not arrays
    try:
        for call in (lambda: dr.duplicates(0), dr.dedup):
            with pytest.raises(native.SpliserNativeError, match="fused"):
                call()
    finally:
        dr.free()
    fine()


def test_the_cases_in_a_child_on_poisoned_memory(wanted, tmp_path):
    """One fresh process, every case, every buffer 0xA5 when handed out: what it gives is what the restatement says, exactly.  The
    child has a time limit and is not started again if it ends badly."""
    out = str(tmp_path / "poisoned")
    env = dict(os.environ, SPL_DEV_POISON="1")
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dup_device.py"), "--out", out], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, universal_newlines=True, timeout=CHILD_TIMEOUT)
        status, said = r.returncode, r.stdout
    except subprocess.TimeoutExpired as e:
        status, said = "none after %d s" % CHILD_TIMEOUT, e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode("utf-8", "replace")
    if status != 0:
        log = os.path.join(out, "progress.log")
        progress = open(log).read().splitlines()[-3:] if os.path.exists(log) else ["(no progress.log)"]
        pytest.fail("the poisoned child ended with exit status %s\n---- its output ----\n%s\n---- it was at ----\n%s"
                    % (status, "\n".join(said.splitlines()[-40:]), "\n".join(progress)), pytrace=False)
    with open(os.path.join(out, "pool.json")) as fh:
        stats = json.load(fh)
    assert stats["handed_out"] > 0 and stats["poisoned"] == stats["handed_out"]
    for name, (_, _, want) in wanted.items():
        with np.load(os.path.join(out, name + ".npz")) as z:
            got = {k: z[k] for k in z.files}
        bad = V.mismatches(got, want)
        assert not bad, "%s, poisoned:\n%s" % (name, "\n".join(bad[:20]))
