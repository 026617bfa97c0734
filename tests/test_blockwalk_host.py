"""The block walk is stated in ``spl_block_walk`` (``csrc/spl_coverage_rule.h``) and has three consumers: ``spl_cov_walk`` (the
walk, clipped, into an emit), ``spl_cov_cursor`` (the same, resumable) and ``spl_exon_hits`` (the walk, not clipped, held against a
map).  EVERY CIGAR of ``blockwalkcases.py`` -- one, two and three ops over eleven codes and the lengths 0, 1, 2 -- goes through
their host hooks (``spl_coverage_rule_host``, ``spl_coverage_cursor_host``, ``spl_exon_count_rule_host``) twice: from p = -1 into a
reference of two bases, where the clipping bites at both ends, and from p = 0 into one no read reaches the end of.  The exon hook
runs over a bin map of width-1 bins of one gene over [0, length): the bins a read hits are exactly its covered bases there.  Each
result is held to the restatement and so to the other two; no case is left out.  The gene fold keeps a loop of its own (the
gene kernel is measurably faster with it: ``csrc/spl_genecount_rule.h``), so ``spl_gene_count_rule_host`` goes through the same
CIGARs, once per base b of [0, length) over a gene map whose one stretch is that base: it says the gene exactly when b is covered.

The hooks take a read a call, so they are called as they are exported, on buffers made once."""
import ctypes

import numpy as np
import pytest

import blockwalkcases as W
from spliser_amd import native


@pytest.fixture(scope="module")
def cigars():
    return W.all_cigars()


def test_the_enumeration_is_complete(cigars):
    assert len(cigars) == 33 + 33 ** 2 + 33 ** 3 == len(set(cigars))
    assert {op & 15 for c in cigars for op in c} == set(W.CODES) and {op >> 4 for c in cigars for op in c} == set(W.LENGTHS)


def test_the_restatement_on_cigars_worked_out_by_hand():
    M, I, D, N, S = (lambda n, c=c: n << 4 | c for c in (0, 1, 2, 3, 4))
    assert W.blocks_of((M(2), I(1), M(1)), 5) == [(5, 8)]                         # an insertion does not part a block
    assert W.blocks_of((M(2), N(0), M(1)), 5) == [(5, 8)]                         # ... nor does a gap of no length
    assert W.blocks_of((M(1), D(1), 1 << 4 | 7), 0) == [(0, 1), (2, 3)]           # a deletion is a gap
    assert W.blocks_of((S(2), N(2), 2 << 4 | 8), -1) == [(1, 3)]                  # a clip does not advance, an intron does
    assert W.blocks_of((2 << 4 | 9, 2 << 4 | 15, 2 << 4 | 6), 0) == []            # codes above 8 and P do nothing
    assert W.clipped([(-1, 3)], 2) == ([(0, 2)], True) and W.clipped([(-1, 0), (1, 2)], 2) == ([(1, 2)], True)
    assert W.clipped([(0, 2)], 2) == ([(0, 2)], False)


@pytest.mark.parametrize("run", [W.CLIPPED, W.UNCLIPPED], ids=["clipped", "unclipped"])
def test_every_cigar_through_the_consumers(cigars, run):
    lib = native.lib()
    length, p = run["length"], run["pos"] - 1 + run["shift"]
    (b_start, b_code), bin_gene = W.width_one_bins(length)
    ops = np.zeros(3, np.uint32)
    s, e, bins = np.zeros(3, np.int64), np.zeros(3, np.int64), np.zeros(8, np.int64)
    n, past, verdict, n_hits = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    flag, pos, shift, zero = ctypes.c_uint32(0), ctypes.c_int32(run["pos"]), ctypes.c_int32(run["shift"]), ctypes.c_int(0)
    cov_args = (shift, ctypes.c_int64(length), zero, zero, ctypes.c_int(3), ptr(s), ptr(e), ctypes.byref(n), ctypes.byref(past))
    exon_args = (shift, zero, ctypes.c_int64(length + 1), ptr(b_start), ptr(b_code), ctypes.c_int64(0), None, None, ctypes.c_int64(length), ptr(bin_gene), ctypes.byref(verdict),
                 ptr(bins), ctypes.c_int64(8), ctypes.byref(n_hits))
    p_ops, counts = ptr(ops), [ctypes.c_uint32(k) for k in range(4)]
    g_code, g_starts, result = np.array([1, 0], np.uint32), [np.array([b, b + 1], np.int32) for b in range(length)], ctypes.c_int64(0)
    gene_args = [(shift, zero, ctypes.c_int64(2), ptr(g), ptr(g_code), ctypes.c_int64(0), None, None, ctypes.c_int64(1), ctypes.byref(result)) for g in g_starts]
    seen = dict(blocks=0, lost=0, both_ends=0, none_left=0)
    for cig in cigars:
        ops[:len(cig)] = cig
        want, want_past = W.clipped(W.blocks_of(cig, p), length)
        for hook in (lib.spl_coverage_rule_host, lib.spl_coverage_cursor_host):
            assert hook(flag, pos, p_ops, counts[len(cig)], *cov_args) == 0
            assert (list(zip(s[:n.value].tolist(), e[:n.value].tolist())), bool(past.value)) == (want, want_past), (hook.__name__, cig)
        assert lib.spl_exon_count_rule_host(flag, pos, p_ops, counts[len(cig)], *exon_args) == 0
        bases = [b for a, z in want for b in range(a, z)]
        assert (verdict.value, bins[:n_hits.value].tolist()) == ((0, bases) if bases else (-1, [])), ("exon", cig)
        for b in range(length):
            assert lib.spl_gene_count_rule_host(flag, pos, p_ops, counts[len(cig)], *gene_args[b]) == 0
            assert result.value == (0 if b in bases else -1), ("gene", cig, b)
        seen["blocks"] += len(want)
        seen["lost"] += want_past
        seen["both_ends"] += any(a < 0 and z > length for a, z in W.blocks_of(cig, p))
        seen["none_left"] += want_past and not want
    assert seen["blocks"] > 10000          # (the cases say something: most CIGARs with an M, = or X of some length leave a block)
    if run is W.CLIPPED:
        assert seen["both_ends"] > 100 and seen["none_left"] > 100
    else:
        assert seen["lost"] == 0
