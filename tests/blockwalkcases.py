"""Shared by ``test_blockwalk_host.py`` and ``test_gpu_blockwalk.py``: EVERY CIGAR of one, two and three ops over the eleven op
codes M I D N S H P = X 9 15 with the lengths 0, 1 and 2 -- 33 + 33^2 + 33^3 = 37 059 reads -- and the block walk restated from the
rule's prose (``csrc/spl_coverage_rule.h``) in a few lines.  Nothing here calls the library; nothing touches the GPU."""
import itertools

import numpy as np

from spliser_amd import samio

CODES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15)          # M I D N S H P = X, and two codes above 8
LENGTHS = (0, 1, 2)
SPAN = 6                                            # bases a read of three ops reaches at most
# The two runs of the host test: p = POS - 1 + shift = -1 into a reference of 2 bases (a block of 4 loses a base at both ends), and
# p = 0 into one no read reaches the end of.
CLIPPED, UNCLIPPED = dict(pos=1, shift=-1, length=2), dict(pos=1, shift=0, length=SPAN + 2)


def all_cigars():
    """-> [tuple of BAM ops]: every CIGAR, the one-op ones first."""
    ops = [n << 4 | c for c in CODES for n in LENGTHS]
    return [cig for k in (1, 2, 3) for cig in itertools.product(ops, repeat=k)]


def blocks_of(ops, p):
    """The rule: M, = and X cover [p, p + len) and advance; D and N advance without covering; every other op, and an op of length
    zero, does nothing; covering ops that abut are one block.  -> [(start, end)], not clipped."""
    out = []
    for op in ops:
        code, n = op & 15, op >> 4
        if n and code in (0, 7, 8):
            if out and out[-1][1] == p:
                out[-1] = (out[-1][0], p + n)
            else:
                out.append((p, p + n))
        if n and code in (0, 2, 3, 7, 8):
            p += n
    return out


def clipped(blocks, length):
    """-> (the blocks clipped to [0, length), those left without a base dropped; whether one lost a base)."""
    cut = [(max(s, 0), min(e, length)) for s, e in blocks]
    return [(s, e) for s, e in cut if e > s], cut != list(blocks)


def width_one_bins(length):
    """A bin map of ``length`` bins of width 1 of one gene over [0, length): the bins a read hits are its covered bases there.
    -> ((start, code), bin_gene)."""
    start = np.arange(length + 1, dtype=np.int32)
    code = np.concatenate((np.arange(1, length + 1), [0])).astype(np.uint32)
    return (start, code), np.zeros(length, np.uint32)


def read_set(cigars, pos, flag, name_key=None):
    """The CIGARs as a ReadSet with these POS and FLAG arrays."""
    n_ops = np.fromiter((len(c) for c in cigars), np.int64, len(cigars))
    cigar = np.fromiter(itertools.chain.from_iterable(cigars), np.uint32, int(n_ops.sum()))
    return samio.ReadSet(pos, flag, np.concatenate(([0], np.cumsum(n_ops))), cigar, name_key=name_key)
