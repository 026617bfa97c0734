"""The position index of an uploaded site table (spl_build_dbuckets_kernel, launched from spl_sites_upload), read back through
spl_sites_index_download and held word for word to the yardstick of indexcases.py -- tables with sites and flagged positions on bit
0 and bit 31 of a bucket, a full bucket, every phase of dbase, dbase = -64, millions of buckets, sites at SPL_COORD_MAX -- and the
index's consumers (the fused range kernel's prologue and span test, the once- and twice-spliced paths, the inline-op path, layout +
range) on those tables against the oracle, through test_gpu_kernel_limits.run_device: every mode, both chunk sizes, fused and not,
counters and SSE bit-equal.  test_indexcases_host.py shows on the CPU that the cases reach the places they name."""
import ctypes

import numpy as np
import pytest

import indexcases as X
from spliser_amd import native
from test_gpu_kernel_limits import run_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


def _assert_words(name, index, first, got):
    want = index.words(first, got.shape[0])
    if np.array_equal(got, want):
        return
    b = int(np.nonzero(np.any(got != want, axis=1))[0][0])
    raise AssertionError("%s: bucket %d (start %d): first, occ, rival = %d, 0x%08x, 0x%08x; the definition gives %d, 0x%08x, 0x%08x"
                         % ((name, first + b, index.start(first + b)) + tuple(int(v) for v in got[b]) + tuple(int(v) for v in want[b])))


def _assert_index(name, index, ds, ranges=None):
    dbase, n_dbuckets, n_dpos, _ = ds.position_index(0, 0)
    assert (dbase, n_dbuckets, n_dpos) == (index.dbase, index.n_dbuckets, index.n_dpos), name
    for first, count in ranges or [(0, n_dbuckets)]:
        got = ds.position_index(first, count)[3]
        assert got.shape == (count, 3) and got.dtype == np.uint32
        _assert_words(name, index, first, got)


# ---- a. the index itself --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in X.TABLES if n != X.BIG])
def test_index_is_the_definition(name, ctx):
    """Every bucket's three words; then the same table uploaded again into the slab the first one gave back."""
    t, index, _ = X.table(name)
    sites = t.sites()
    with ctx.upload_sites(sites) as ds:
        _assert_index(name, index, ds)
        first = ds.position_index()
    with ctx.upload_sites(sites) as ds:
        again = ds.position_index()
    assert first[:3] == again[:3] and np.array_equal(first[3], again[3]), name


def test_index_of_67_million_buckets(ctx):
    """Sites at 0 and at SPL_COORD_MAX in one table (805 MB of index), read back in ranges: the first and the last 4096 buckets and
    64 buckets around every site and flagged position."""
    t, index, _ = X.table(X.BIG)
    with ctx.upload_sites(t.sites()) as ds:
        _assert_index(X.BIG, index, ds, X.ranges_to_read(index))


def test_refusals_of_the_read_back(ctx):
    t, index, _ = X.table("phase_1")
    lib, n = native.lib(), index.n_dbuckets
    out = np.zeros((n + 1, 3), np.uint32)
    with ctx.upload_sites(t.sites()) as ds:
        u32 = ctypes.c_uint32
        for args in ((ctx._h, ds._h, u32(0), u32(n + 1), native._ptr(out)), (ctx._h, ds._h, u32(n), u32(1), native._ptr(out)),
                     (ctx._h, ds._h, u32(1), u32(n), native._ptr(out)), (ctx._h, ds._h, u32(0xffffffff), u32(2), native._ptr(out)),
                     (ctx._h, ds._h, u32(2), u32(0xffffffff), native._ptr(out)),
                     (None, ds._h, u32(0), u32(1), native._ptr(out)), (ctx._h, None, u32(0), u32(1), native._ptr(out)),
                     (ctx._h, ds._h, u32(0), u32(1), None)):
            assert lib.spl_sites_index_download(*args) == -1, args[2:4]
        assert lib.spl_sites_index_info(None, None, None, None) == -1
        assert not out.any()
        with pytest.raises(native.SpliserNativeError):
            ds.position_index(n, 1)
        assert ds.position_index(n, 0)[3].shape == (0, 3)
        _assert_index("phase_1", index, ds)                      # the context and the table still work
        _assert_index("phase_1", index, ds, [(n - 1, 1), (3, 2)])


# ---- b. the consumers -----------------------------------------------------------------------------------------------------------

def _run(name, shift, ctx, oracle_lib, monkeypatch):
    case = X.consumer_case(name, shift)
    X.assert_named_rows_count(oracle_lib, case)
    run_device(ctx, oracle_lib, monkeypatch, case)


@pytest.mark.parametrize("name", X.CONSUMER_CASES)
def test_consumers_on_the_edges_of_the_index(name, ctx, oracle_lib, monkeypatch):
    _run(name, 0, ctx, oracle_lib, monkeypatch)


def test_consumers_below_the_coordinate_limit(ctx, oracle_lib, monkeypatch):
    """`top`: the reads around its sites are added with a shift just below 2^31, the last site is SPL_COORD_MAX."""
    _run("top", X.TOP_SHIFT, ctx, oracle_lib, monkeypatch)
