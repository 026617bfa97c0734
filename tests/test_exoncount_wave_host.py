"""How a wave of ``spl_exon_count`` adds its 64 reads' bins and verdicts to the counts (spliser_amd/csrc/spl_exoncount_wave.h: the
body the kernel of spl_exoncount.hip calls every step) built for the host against tests/hostsim/wave_emul.h -- a wave = 64 fibers,
every cross-lane primitive a checked rendezvous -- and held against plain loops: the bins' sums, the four verdict counters, and the
adds themselves, one per run of equal bins in lane order in every ROUND (round j: every lane's j-th bin).  The reference has no
such step: it counts no exon bins."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import exoncases as X

HERE = os.path.dirname(os.path.abspath(__file__))
COUNTED, NO_FEATURE, AMBIGUOUS, NOT_COUNTED = 0, 1, 2, 3      # spl_exoncount_rule.h's verdicts: the index of a read's counter


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(HERE, "hostsim", "libexoncount_wave_host.so")
    csrc = os.path.join(HERE, "..", "spliser_amd", "csrc")
    srcs = [os.path.join(HERE, "hostsim", "exoncount_wave_host.cpp"), os.path.join(HERE, "hostsim", "wave_emul.h"), os.path.join(csrc, "spl_exoncount_wave.h"),
            os.path.join(csrc, "spl_genecount_wave.h"), os.path.join(csrc, "spl_wave.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
    return ctypes.CDLL(so)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run(lib, reads, n_bins):
    """reads: [(verdict, [bins])] -> (counts[n_bins], tallies[4], the adds as a sorted list of (bin, value))."""
    verdicts = np.array([v for v, _ in reads], np.uint32)
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for _, b in reads])
    bins = np.array([x for _, b in reads for x in b] + [0], np.uint32)
    counts, tallies = np.zeros(max(n_bins, 1), np.uint64), np.zeros(4, np.uint64)
    adds, n_adds = np.zeros(2 * max(len(bins), 1), np.uint64), ctypes.c_uint64(0)
    rc = lib.exoncount_wave_run(_ptr(verdicts), _ptr(off), _ptr(bins), ctypes.c_uint64(len(reads)), ctypes.c_uint32(n_bins), _ptr(counts), _ptr(tallies), _ptr(adds),
                                ctypes.c_uint64(len(adds) // 2), ctypes.byref(n_adds))
    assert rc == 0, "the wave broke a rule of the emulator (%d)" % rc
    pairs = adds[:2 * n_adds.value].reshape(-1, 2).tolist()
    return counts[:n_bins].tolist(), tallies.tolist(), sorted((int(b), int(v)) for b, v in pairs)


def want(reads, n_bins):
    """Plain loops: the sums, and per wave and round one add per run of equal bins in lane order (a lane with no bin left ends a run)."""
    counts, tallies, adds = [0] * n_bins, [0, 0, 0, 0], []
    for v, bins in reads:
        tallies[v] += 1
        for b in bins:
            counts[b] += 1
    for base in range(0, len(reads), 64):
        lists = [b for _, b in reads[base:base + 64]]
        for j in range(max(len(b) for b in lists)):
            before = None
            for b in lists:
                cur = b[j] if j < len(b) else None
                if cur is not None:
                    if cur != before:
                        adds.append([cur, 0])
                    adds[-1][1] += 1
                before = cur
    return counts, tallies, sorted((b, v) for b, v in adds)


def both(lib, reads, n_bins):
    got = run(lib, reads, n_bins)
    assert got == want(reads, n_bins)
    as_yardstick = [(-v, b) for v, b in reads]
    assert (len(got[2]), sum(len(b) for _, b in reads)) == X.adds_of(as_yardstick)          # the measurement's count of adds is this rule
    assert got[0] + got[1] == X.counts_of(as_yardstick, None, n_bins)
    return got


def test_all_lanes_one_bin_is_one_add_of_64(lib):
    counts, tallies, adds = both(lib, [(COUNTED, [5])] * 64, 9)
    assert adds == [(5, 64)] and counts[5] == 64 and tallies == [64, 0, 0, 0]


def test_a_different_bin_every_lane_is_64_adds(lib):
    counts, _, adds = both(lib, [(COUNTED, [k]) for k in range(64)], 64)
    assert adds == [(k, 1) for k in range(64)] and counts == [1] * 64


def test_lanes_with_0_1_2_and_70_bins_in_one_wave(lib):
    """The wave goes on for 70 rounds; from the third on one lane alone has a bin."""
    seventy = list(range(10, 80))
    reads = [(NO_FEATURE, []), (COUNTED, [10]), (COUNTED, [10, 11]), (COUNTED, seventy), (AMBIGUOUS, []), (COUNTED, [10, 11])] + [(COUNTED, [10])] * 58
    counts, tallies, adds = both(lib, reads, 80)
    assert tallies == [62, 1, 1, 0] and counts[10] == 62 and counts[11] == 3 and counts[12:] == [1] * 68
    # round 0: lanes 1..3 and 5..63 offer bin 10 (lane 0 and lane 4 cut the run); round 1: 11 from lanes 2..3 and from lane 5
    assert adds == sorted([(10, 3), (10, 59), (11, 2), (11, 1)] + [(b, 1) for b in range(12, 80)])


@pytest.mark.parametrize("where", [0, 63])
def test_a_read_of_70_bins_beside_one_bin_reads(lib, where):
    reads = [(COUNTED, [3])] * 64
    reads[where] = (COUNTED, list(range(70)))
    counts, _, adds = both(lib, reads, 70)
    assert counts[3] == 64 and sum(counts) == 63 + 70 and len(adds) == 2 + 69          # round 0: two runs; 69 rounds of one lane


@pytest.mark.parametrize("idle", [(0, 5), (59, 64), (0, 64), (1, 63)])
def test_idle_lanes_at_either_end(lib, idle):
    """Lanes whose reads have no bin (not counted, no feature): they end a run and add nowhere."""
    reads = [(NOT_COUNTED, []) if idle[0] <= k < idle[1] else (COUNTED, [2, 4]) for k in range(64)]
    n = 64 - (idle[1] - idle[0])
    counts, tallies, adds = both(lib, reads, 5)
    assert counts == [0, 0, n, 0, n] and tallies == [n, 0, 0, 64 - n]
    assert len(adds) == (0 if n == 0 else 4 if idle == (1, 63) else 2)


@pytest.mark.parametrize("n", [1, 2, 37, 63, 65, 130])
def test_a_wave_that_is_not_full(lib, n):
    counts, tallies, adds = both(lib, [(COUNTED, [1, 2])] * n, 3)
    assert counts == [0, n, n] and tallies == [n, 0, 0, 0]
    assert adds == sorted((b, min(64, n - base)) for base in range(0, n, 64) for b in (1, 2))


def test_a_bin_beyond_the_bins_is_counted_nowhere(lib):
    """There is none (the maps' codes are checked); said for the memory's sake."""
    counts, _, adds = run(lib, [(COUNTED, [0, 2]), (COUNTED, [1, 2]), (COUNTED, [5])], 2)
    assert counts == [1, 1] and adds == [(0, 1), (1, 1)]


def test_random_reads_over_many_waves(lib):
    rng = np.random.default_rng(20261020)
    n_bins = 40
    for n, p_change in ((64 * 7 + 13, 0.05), (64 * 5, 0.5), (700, 1.0)):
        reads, cur = [], (COUNTED, [0])
        for _ in range(n):
            if rng.random() < p_change:
                v = int(rng.choice([COUNTED, NO_FEATURE, AMBIGUOUS, NOT_COUNTED], p=[0.7, 0.1, 0.1, 0.1]))
                first = int(rng.integers(0, n_bins - 6))
                cur = (v, list(range(first, first + int(rng.integers(1, 6)))) if v == COUNTED else [])
            reads.append(cur)
        counts, tallies, adds = both(lib, reads, n_bins)
        assert sum(tallies) == n and sum(v for _, v in adds) == sum(counts)
