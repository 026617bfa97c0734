"""The fused range kernel asks ONE pair of position-index entries for all the simple reads of a thread (spl_simple_span.h: the
span test) and looks only at the reads of the threads whose span holds a site.  The rule on the host (spl_simple_span_host: the
header the kernel includes, over an index laid out and filled as the device's is) against a plain restatement with numpy's
searchsorted: a thread that is not flagged has no read that counts for anything, and a flagged thread's reads get the ranges the
restatement gives -- for any mix of simple and other reads, in any order of position, lengths 1 .. 65535, left of, right of and
across the ends of the table."""
import numpy as np
import pytest

from spliser_amd import native

COORD_MAX = 2147483581


@pytest.fixture(scope="module", autouse=True)
def built():
    native.build()


def restate(site_pos, pos, length, is_simple, shift):
    """Per read: [lo, ub) = the distinct site positions t with t and t + 1 both among the bases [a, b), a = pos + shift, b = a + length:
    lo = sites <= a - 1, ub = sites < b - 1."""
    a = pos.astype(np.int64) + shift
    b = a + length.astype(np.int64)
    lo = np.searchsorted(site_pos, a - 1, side="right")
    ub = np.searchsorted(site_pos, b - 1, side="left")
    return lo, ub, (ub > lo) & is_simple.astype(bool)


def check(site_pos, pos, length, is_simple, shift=0, rpt=4):
    site_pos = np.asarray(site_pos, np.int64)
    pos, length, is_simple = np.asarray(pos, np.int64), np.asarray(length, np.int64), np.asarray(is_simple, bool)
    flagged, emits, lo, ub = native.simple_span_host(site_pos, pos, length, is_simple, shift, rpt)
    want_lo, want_ub, want_emit = restate(site_pos, pos, length, is_simple, shift)
    per_thread = np.repeat(flagged, rpt)
    # a thread that is not flagged has no emitting read
    assert not np.any(want_emit & ~per_thread)
    # a flagged thread's simple reads: the restatement's ranges
    listed = per_thread & is_simple
    assert np.array_equal(lo[listed], want_lo[listed]) and np.array_equal(ub[listed], want_ub[listed])
    assert np.array_equal(emits, want_emit)
    # nothing is said about the other reads
    assert not emits[~listed].any() and not lo[~listed].any() and not ub[~listed].any()
    # a thread without a simple read is never flagged
    assert not np.any(flagged & ~is_simple.reshape(-1, rpt).any(axis=1))
    return flagged, want_emit


def test_two_reads_150_bases_apart_with_a_site_between_them():
    """What the list is for: the span holds the site, no read does -- flagged, nothing emits."""
    flagged, emit = check([10000], [9800, 10050, 9800, 9800], [100, 100, 100, 100], [1, 1, 0, 0])
    assert flagged.tolist() == [True] and not emit.any()
    flagged, emit = check([10000], [9800, 10050, 9950, 9800], [100, 100, 100, 100], [1, 1, 0, 0])
    assert flagged.tolist() == [True] and not emit.any()         # (the read over the site is not a simple one)
    flagged, emit = check([10000], [9800, 10050, 9950, 9800], [100, 100, 100, 100], [1, 1, 1, 0])
    assert flagged.tolist() == [True] and emit.tolist() == [False, False, True, False]


def test_site_on_a_reads_first_and_last_bases():
    """A site t counts when t and t + 1 both lie under the read: a <= t and t + 1 <= b - 1."""
    t = 5000
    pos = [t, t - 49, t - 50, t - 1, t - 48, t + 1, t, t]
    length = [50, 50, 50, 2, 50, 50, 1, 2]
    flagged, emit = check([t], pos, length, [1] * 8)
    assert emit.tolist() == [True, False, False, False, True, False, False, True]
    flagged, emit = check([t], pos, length, [1] * 8, rpt=1)
    assert flagged.tolist() == emit.tolist()                       # one read a thread: the span is the read


@pytest.mark.parametrize("seed", range(6))
def test_random_threads(seed):
    rng = np.random.default_rng(seed)
    n_sites = int(rng.integers(1, 400))
    first = int(rng.choice([0, 3, 64, 65, 1000, 50000]))
    gaps = rng.choice([1, 2, 3, 7, 31, 32, 33, 150, 4000], n_sites)
    site_pos = first + np.cumsum(gaps) - gaps[0]
    lo_t, hi_t = int(site_pos[0]), int(site_pos[-1])
    n = 4 * 5000
    # positions left of the table, across its ends, inside and right of it; in no order
    pos = rng.integers(max(0, lo_t - 70000), hi_t + 70000, n)
    near = rng.random(n) < 0.3
    pos[near] = rng.choice(site_pos, int(near.sum())) + rng.integers(-3, 4, int(near.sum()))
    pos = np.maximum(pos, 0)
    length = rng.choice([1, 2, 3, 50, 100, 151, 65535], n)
    wild = rng.random(n) < 0.3
    length[wild] = rng.integers(1, 65536, int(wild.sum()))
    is_simple = rng.random(n) < float(rng.choice([0.2, 0.6, 1.0]))
    flagged, emit = check(site_pos, pos, length, is_simple)
    assert flagged.any() and not flagged.all() or n_sites < 3
    # the same reads two and one a thread, and in descending order within every thread
    check(site_pos, pos, length, is_simple, rpt=2)
    order = np.argsort(-pos.reshape(-1, 4), axis=1, kind="stable")
    idx = (np.arange(n // 4)[:, None] * 4 + order).ravel()
    check(site_pos, pos[idx], length[idx], is_simple[idx])


def test_a_segments_shift_and_the_top_of_the_coordinate_space():
    sites = [COORD_MAX - 40000, COORD_MAX - 100, COORD_MAX - 1, COORD_MAX]
    shift = 1000000
    pos = np.array([COORD_MAX - 65535, COORD_MAX - 50, COORD_MAX - 2, COORD_MAX - 120, 0, 5, COORD_MAX - 40001, COORD_MAX - 1]) - shift
    length = [65535, 50, 2, 100, 65535, 1, 3, 1]
    flagged, emit = check(sites, pos, length, [1] * 8, shift=shift)
    assert emit.tolist() == [True, False, False, True, False, False, True, False]
    with pytest.raises(native.SpliserNativeError):
        native.simple_span_host(sites, [COORD_MAX - 10 - shift] * 4, [11] * 4, [1] * 4, shift)


def test_dense_sites_flag_every_thread():
    sites = 40000 + 3 * np.arange(1500)
    pos = 40000 + np.arange(4 * 256) * 4
    flagged, emit = check(sites, pos, np.full(pos.shape, 60), np.ones(pos.shape, bool))
    assert flagged.all() and emit.all()
