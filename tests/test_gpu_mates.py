"""The mate table on the device (``spl_mate_table``: compaction, eight passes of the radix sort, the pair kernel) against the
yardstick of ``matecases.py``, exactly, through ``upload_soa`` with the keys given directly -- equal keys need no hash collision --
at the sizes where the kernels' geometry changes, on groups of every shape, on keys that differ in one byte or one bit, on reads
that are not pairable under a pair's key, per segment of a set of several, and its refusal of a set without keys."""
import numpy as np
import pytest

import matecases as M
from spliser_amd import native, samio

pytestmark = pytest.mark.gpu

# The kernels' geometry (csrc/spl_mates.h): a workgroup takes SPL_MATE_TILE = 256 reads (elements) a grid-stride step, one a lane,
# and a launch has at most SPL_MATE_GRID_MAX = 1024 workgroups: EVERY workgroup of the mark, the compaction and the pair kernel takes
# a second step from 2 * 1024 * 256 - 255 pairable reads on.
TILE, GRID_MAX = 256, 1024
LARGE = 2 * GRID_MAX * TILE + 1


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


def _reads(flag, pos=None, n_ops=None):
    """Reads of one aligned op (or of none where n_ops says 0), at POS 1, 2, ... unless told."""
    n = len(flag)
    n_ops = np.ones(n, np.int64) if n_ops is None else np.asarray(n_ops, np.int64)
    return samio.ReadSet(np.arange(1, n + 1) if pos is None else pos, np.asarray(flag, np.uint16), np.concatenate(([0], np.cumsum(n_ops))), np.full(int(n_ops.sum()), (20 << 4), np.uint32))


def _tables(ctx, sets):
    """[(ReadSet, keys)] as the segments of one fused set -> [(mate list, counts)] per segment."""
    arrays = [native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, name_key=keys) for rs, keys in sets]
    with ctx.upload_soa(arrays, with_keys=True) as soa:
        with ctx.begin_reads() as dr:
            for k in range(len(sets)):
                dr.add_soa(soa, k, 1000 * k)
            dr.finish()
            assert dr.has_mate_keys() or not sum(rs.n for rs, _ in sets)
            out, seg = [], 0          # (a segment without a read is none of the set's)
            for rs, _ in sets:
                mate, counts = dr.mate_table(seg, rs.n) if rs.n or len(sets) == 1 else (np.zeros(0, np.uint32), dict.fromkeys(native.MATE_COUNTS, 0))
                seg += 1 if rs.n else 0
                out.append((mate.tolist(), counts))
            again = dr.mate_table(0, sets[0][0].n)          # (kept with the set: the same table)
            assert again[0].tolist() == out[0][0] and again[1] == out[0][1]
            return out


def _check(ctx, rs, keys):
    keys = np.asarray(keys, np.uint64)
    want = M.mate_table_of(rs, keys)
    got = _tables(ctx, [(rs, keys)])[0]
    assert got[1] == want[1]
    assert got[0] == want[0]
    return want


def _mixed(rng, n_pairable, spoil=True):
    """n_pairable pairable reads -- pairs 99/147 under random keys, the odd one alone -- among reads that are not: flag and keys."""
    n_pairs = n_pairable // 2
    keys = rng.integers(1, 2 ** 63, n_pairs + 1, dtype=np.uint64) << np.uint64(1)
    flag = [99] * n_pairs + [147] * n_pairs + [99] * (n_pairable - 2 * n_pairs)
    k = list(keys[:n_pairs]) * 2 + [keys[n_pairs]] * (n_pairable - 2 * n_pairs)
    if spoil:
        extra = max(3, n_pairable // 5)
        flag += [0, 16, 99 | 256, 147 | 2048, 1 | 64 | 128, 1 | 4 | 64, 99 | 512][:extra] * 1 + [0] * max(0, extra - 7)
        k += [keys[i % (n_pairs + 1)] for i in range(len(flag) - len(k))]
    perm = rng.permutation(len(flag))
    return np.array(flag, np.uint16)[perm], np.array(k, np.uint64)[perm]


# ---- sizes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2])
def test_sets_of_no_one_and_two_reads(ctx, n):
    want = _check(ctx, _reads([99, 147][:n]), [10, 11][:n])
    assert want[1]["paired"] == (2 if n == 2 else 0)


@pytest.mark.parametrize("n_pairable", [63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_pairable_counts_around_a_wave_and_a_tile(ctx, n_pairable):
    flag, keys = _mixed(np.random.default_rng(n_pairable), n_pairable)
    want = _check(ctx, _reads(flag), keys)
    assert want[1]["pairable"] == n_pairable and want[1]["paired"] == n_pairable // 2 * 2


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1])
def test_reads_around_a_tile_with_few_pairable(ctx, n):
    """The mark and the compaction kernel's tile is over the READS: n reads of which ten are pairable, the last one among them."""
    flag = np.zeros(n, np.uint16)
    keys = np.arange(1, n + 1, dtype=np.uint64) << np.uint64(8)
    at = [0, 1, 62, 63, 64, 65, n - 3, n - 2, n - 1, n // 2]
    flag[at] = [99, 147] * 5
    keys[at] = np.repeat(np.array([2, 4, 6, 8, 10], np.uint64), 2)
    want = _check(ctx, _reads(flag), keys)
    assert want[1] == dict(pairable=10, paired=10, unpaired_mate_mapped=0)


def test_a_set_that_gives_every_workgroup_of_every_kernel_a_second_step(ctx):
    """LARGE reads, all pairable: half a million pairs under random keys, every other pair adjacent, the rest anywhere in the set's
    second half -- most of them farther apart than many tiles."""
    rng = np.random.default_rng(11)
    n_pairs = LARGE // 2
    keys = np.empty(LARGE, np.uint64)
    flag = np.empty(LARGE, np.uint16)
    pair_keys = (rng.permutation(n_pairs).astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) & np.uint64(0xFFFFFFFFFFFFFFFE)   # distinct, all bytes in use
    assert np.unique(pair_keys >> np.uint64(1)).shape[0] == n_pairs
    near = n_pairs // 2
    keys[0:2 * near:2], keys[1:2 * near:2] = pair_keys[:near], pair_keys[:near]          # neighbours
    flag[0:2 * near:2], flag[1:2 * near:2] = 99, 147
    rest = np.arange(2 * near, LARGE)
    where = rng.permutation(rest)
    far = n_pairs - near
    keys[where[:far]], keys[where[far:2 * far]] = pair_keys[near:], pair_keys[near:]
    flag[where[:far]], flag[where[far:2 * far]] = 83, 163
    keys[where[2 * far:]] = np.uint64(2)                                                     # the odd one: alone
    flag[where[2 * far:]] = 73
    want = _check(ctx, _reads(flag), keys)
    assert want[1] == dict(pairable=LARGE, paired=LARGE - 1, unpaired_mate_mapped=0)
    m = np.array(want[0], np.int64)
    gap = np.abs(m[:-1] - np.arange(LARGE - 1))
    assert (gap == 1).sum() >= near and (gap[m[:-1] != M.NONE] > 64 * TILE).sum() > 100000


# ---- groups -------------------------------------------------------------------------------------------------------------------
def test_all_reads_under_one_key_with_unequal_halves(ctx):
    rng = np.random.default_rng(5)
    flag = np.where(rng.random(3000) < 0.37, 99, 147).astype(np.uint16)
    want = _check(ctx, _reads(flag), np.full(3000, 0xDEADBEEF12345678, np.uint64))
    n_first = int((flag == 99).sum())
    assert want[1] == dict(pairable=3000, paired=2 * min(n_first, 3000 - n_first), unpaired_mate_mapped=3000 - 2 * min(n_first, 3000 - n_first))


def test_groups_of_two_and_two_and_of_three_and_one(ctx):
    flag = [99, 99, 147, 147, 65, 99, 147, 99, 163]
    keys = [40, 40, 40, 40, 90, 90, 90, 90, 7000]
    want = _check(ctx, _reads(flag), keys)
    assert want[0] == [2, 3, 0, 1, 6, M.NONE, 4, M.NONE, M.NONE]
    assert want[1] == dict(pairable=9, paired=6, unpaired_mate_mapped=3)


def test_the_least_and_the_greatest_key_and_keys_that_differ_in_one_byte(ctx):
    """Key 1 and key 2^64 - 1 are groups of their own (bit 0 is the kind's); for every byte of the key a pair of groups that differ
    in that byte alone: a sort that skipped a pass would merge them."""
    keys, flag = [1, 1, 2 ** 64 - 1, 2 ** 64 - 1], [99, 147, 147, 99]
    base = 0x4142434445464748
    for byte in range(8):
        for k in (base, base ^ (0x80 << (8 * byte)), base ^ (0x02 << (8 * byte))):
            keys += [k, k]
            flag += [99, 147]
    rng = np.random.default_rng(2)
    perm = rng.permutation(len(keys))
    keys, flag = np.array(keys, np.uint64)[perm], np.array(flag, np.uint16)[perm]
    want = _check(ctx, _reads(flag), keys)
    assert want[1]["paired"] == len(keys)
    m = want[0]
    assert all(int(keys[i]) >> 1 == int(keys[m[i]]) >> 1 for i in range(len(m)))
    assert len({int(k) >> 1 for k in keys}) == 2 + 17


def test_keys_that_differ_in_bit_0_only_are_one_group(ctx):
    want = _check(ctx, _reads([99, 147, 99, 147]), [500, 501, 503, 502])
    assert want[0] == [1, 0, 3, 2]


def test_reads_that_are_not_pairable_under_a_pairs_key(ctx):
    """Secondary, supplementary, QC-failed, unmapped, unpaired, both or neither of 0x40 / 0x80, POS 0, no CIGAR, key 0: each shares
    the key of a proper pair and stands between its mates."""
    spoilers = [(99 | 256, 5, 1), (147 | 2048, 5, 1), (99 | 512, 5, 1), (1 | 4 | 64, 5, 1), (0, 5, 1), (16, 5, 1), (1 | 64 | 128, 5, 1), (1, 5, 1), (99, 0, 1), (147, 5, 0)]
    flag, pos, n_ops, keys = [], [], [], []
    for k, (f, p, o) in enumerate(spoilers):
        key = 1000 + 2 * k
        flag += [99, f, 147]; pos += [5, p, 5]; n_ops += [1, o, 1]; keys += [key] * 3
    flag += [99, 147]; pos += [5, 5]; n_ops += [1, 1]; keys += [0, 0]          # a pair without a name
    want = _check(ctx, _reads(flag, np.array(pos), n_ops), keys)
    assert want[1] == dict(pairable=2 * len(spoilers), paired=2 * len(spoilers), unpaired_mate_mapped=0)
    assert all(want[0][3 * k] == 3 * k + 2 and want[0][3 * k + 1] == M.NONE for k in range(len(spoilers))) and want[0][-2:] == [M.NONE, M.NONE]


def test_a_generated_set_of_every_kind(ctx):
    rng = np.random.default_rng(20261020)
    records, names, kinds = M.paired_records(rng, 400, 5000)
    rs = samio.ReadSet.from_records(records)
    keys = np.array([M.name_key(n) for n in names], np.uint64)
    M.assert_covers(kinds, rs.flag, rs.pos, np.diff(rs.cig_off.astype(np.int64)), keys)
    want = _check(ctx, rs, keys)
    assert 0 < want[1]["unpaired_mate_mapped"] and want[1]["paired"] < want[1]["pairable"] < rs.n


# ---- segments -----------------------------------------------------------------------------------------------------------------
def test_indexes_are_per_segment_and_a_name_on_two_segments_is_two_singletons(ctx):
    rng = np.random.default_rng(8)
    sets = []
    for n_pairable in (300, 0, 1, 777):
        flag, keys = _mixed(rng, n_pairable, spoil=n_pairable > 1)
        sets.append((_reads(flag), keys))
    sets.append((_reads([]), np.zeros(0, np.uint64)))                                        # a segment without a read
    sets.append((_reads([99]), np.array([4242], np.uint64)))
    sets.append((_reads([147]), np.array([4242], np.uint64)))                                # its mate, on another chromosome
    got = _tables(ctx, sets)
    for (rs, keys), (mate, counts) in zip(sets, got):
        want = M.mate_table_of(rs, keys)
        assert mate == want[0] and counts == want[1]
    assert got[-1][0] == [M.NONE] and got[-2][0] == [M.NONE] and got[-1][1]["unpaired_mate_mapped"] == 1


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_a_set_without_keys_is_refused_and_the_context_goes_on(ctx):
    rs = _reads([99, 147])
    arrays = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)
    with ctx.upload_soa([arrays]) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            assert not dr.has_mate_keys()
            for call in (lambda: dr.mate_table(0, 2), lambda: dr.gene_counts(1, None, fragments=True)):
                with pytest.raises(native.SpliserNativeError, match="name keys") as err:
                    call()
                assert err.value.code == -1
            assert dr.gene_counts(1, None).tolist() == [0, 2, 0, 0]
    dr = ctx.upload_reads(arrays)                  # (packed on the host: records, not arrays)
    try:
        with pytest.raises(native.SpliserNativeError, match="fused"):
            dr.mate_table(0, 2)
    finally:
        dr.free()
    with pytest.raises(ValueError, match="name_key"):
        ctx.upload_soa([arrays], with_keys=True)
    _check(ctx, rs, [6, 6])
    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, name_key=np.array([6, 6], np.uint64))], with_keys=True) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            with pytest.raises(native.SpliserNativeError, match="segment"):
                dr.mate_table(1, 2)
