"""``spl_reads_subsample`` on the device against the restatement of ``subsamplecases.py``, exactly, through ``upload_soa`` with the keys
given directly -- a test says which read is kept -- at the sizes where the kernels' geometry changes (a wave, a tile, more than one
tile), on every pattern of kept reads, on CIGARs of no op and of thousands at a tile's edge, over segments, on a key of 0, twice
over; every carried array is held by a consumer of the selected set (``subsample_device.py``).  Its refusals leave the context
usable.  The same cases once more in one fresh child process on poisoned device memory (``SPL_DEV_POISON=1``)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import subsample_device as D
import subsamplecases as S
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
    out = {}
    for name, segs, seed, threshold, with_strand in D.case_list(tile):
        site = D.site_arrays(ctx, segs)
        out[name] = (segs, seed, threshold, with_strand, site, D.want_of(ctx, segs, seed, threshold, with_strand, site))
    return out


PARTS = 8          # the cases in eight tests, a few seconds each


@pytest.mark.parametrize("part", range(PARTS))
def test_cases(ctx, wanted, part):
    seen = 0
    for k, (name, (segs, seed, threshold, with_strand, site, want)) in enumerate(wanted.items()):
        if k % PARTS != part:
            continue
        bad = D.mismatches(D.got_of(ctx, segs, seed, threshold, with_strand, site), want)
        assert not bad, "%s:\n%s" % (name, "\n".join(bad[:20]))
        seen += 1
    assert seen


def test_the_cases_are_the_issues(tile):
    names = {n for n, _, _, _, _ in D.case_list(tile)}
    for n in S.sizes(tile):
        for p in ("all", "none") + (("first", "last", "alternate", "random") if n else ()) + (("run",) if n > tile else ()):
            assert {"n%d_%s_xs" % (n, p), "n%d_%s_plain" % (n, p)} <= names
    assert {"no_ops_kept_xs", "no_ops_dropped_plain", "long_300_kept_xs", "long_5000_kept_plain", "long_5000_dropped_xs", "empty_middle_xs", "loses_every_read_plain",
            "boundary_in_a_tile_xs", "key_0_plain", "pairs_xs"} <= names


def test_a_selection_of_a_selection_is_the_smaller_selection(ctx, tile):
    rng = np.random.default_rng(21)
    n = 2 * tile + 50
    rs = S.reads_of(S.mixed_kinds(n, rng), rng.integers(0, 2 ** 63, n, dtype=np.uint64), rng)
    t1, t2 = S.ALL // 4, (3 * S.ALL) // 4
    length = D.length_of([rs])
    with D.fused(ctx, [rs], True) as dr:
        big, kept2 = dr.subsample(3, t2)
        try:
            small, kept1, index = big.subsample(3, t1, with_index=True)
            try:
                got = D.views(ctx, small, [int(kept1[0])], True, length, None)
            finally:
                small.free()
            direct, kept_direct = dr.subsample(3, t1)
            try:
                want = D.views(ctx, direct, [int(kept_direct[0])], True, length, None)
            finally:
                direct.free()
        finally:
            big.free()
        every, kept_all = dr.subsample(3, S.ALL)
        every.free()
    assert kept_all.tolist() == [n] and kept1.tolist() == kept_direct.tolist() == [int(rs.mask(3, t1).sum())] and kept2.tolist() == [int(rs.mask(3, t2).sum())]
    assert not D.mismatches(got, want)
    m2 = rs.mask(3, t2)
    assert np.array_equal(index, np.flatnonzero(rs.masked(m2).mask(3, t1)))


def test_the_same_words_from_run_to_run(ctx, tile):
    rng = np.random.default_rng(22)
    n = 3 * tile + 5
    rs = S.reads_of(S.mixed_kinds(n, rng), rng.integers(0, 2 ** 63, n, dtype=np.uint64), rng)
    with D.fused(ctx, [rs], True) as dr:
        runs = []
        for _ in range(3):
            sel, kept, index = dr.subsample(1, S.ALL // 2, with_index=True)
            try:
                runs.append((kept.tolist(), index.tobytes(), D.views(ctx, sel, [int(kept[0])], True, D.length_of([rs]), None)))
            finally:
                sel.free()
    for r in runs[1:]:
        assert r[0] == runs[0][0] and r[1] == runs[0][1] and not D.mismatches(r[2], runs[0][2])


def test_refusals_leave_the_context_usable(ctx):
    rng = np.random.default_rng(23)
    rs = S.reads_of(["plain", "once", "plain"], np.array([5, 6, 7], np.uint64), rng)
    plain = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)

    def fine():
        with D.fused(ctx, [rs], False) as dr:
            sel, kept = dr.subsample(0, S.ALL)
            sel.free()
            assert kept.tolist() == [3]

    with D.fused(ctx, [rs], False) as dr:
        with pytest.raises(native.SpliserNativeError, match="2\\^32") as err:
            dr.subsample(0, S.ALL + 1)
        assert err.value.code == -1
    fine()
    with ctx.upload_soa([plain]) as soa:          # no keys
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            with pytest.raises(native.SpliserNativeError, match="name keys") as err:
                dr.subsample(0, 5)
            assert err.value.code == -1
    fine()
    with ctx.upload_soa([D._arrays(rs, False)], with_keys=True) as soa:          # not finished
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            with pytest.raises(native.SpliserNativeError, match="not finished") as err:
                dr.subsample(0, 5)
            assert err.value.code == -1
    fine()
    dr = ctx.upload_reads(plain)          # packed on the host: records, not arrays
    try:
        with pytest.raises(native.SpliserNativeError, match="fused"):
            dr.subsample(0, 5)
    finally:
        dr.free()
    fine()


def test_the_cases_in_a_child_on_poisoned_memory(wanted, tmp_path):
    """One fresh process, every case, every buffer 0xA5 when handed out: what it gives is what the restatement says, exactly.  The
    child has a time limit and is not started again if it ends badly."""
    out = str(tmp_path / "poisoned")
    env = dict(os.environ, SPL_DEV_POISON="1")
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "subsample_device.py"), "--out", out], cwd=ROOT, env=env, stdout=subprocess.PIPE,
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
    for name, (_, _, _, _, _, want) in wanted.items():
        with np.load(os.path.join(out, name + ".npz")) as z:
            got = {k: z[k] for k in z.files}
        bad = D.mismatches(got, want)
        assert not bad, "%s, poisoned:\n%s" % (name, "\n".join(bad[:20]))
