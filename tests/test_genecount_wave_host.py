"""How a wave of ``spl_gene_count`` adds its 64 results to the gene counts (spliser_amd/csrc/spl_genecount_wave.h: the body the
kernel of spl_genecount.hip calls every step) built for the host against tests/hostsim/wave_emul.h -- a wave = 64 fibers, every
cross-lane primitive a checked rendezvous -- and held against plain loops: the counts, the three special counters, and the adds
themselves, one per run of equal gene results in lane order.  The reference has no such step: it counts no genes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import genecases as G

HERE = os.path.dirname(os.path.abspath(__file__))
NO_FEATURE, AMBIGUOUS, NOT_COUNTED, IDLE = 0xFFFFFFFC, 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF      # spl_genecount_rule.h


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(HERE, "hostsim", "libgenecount_wave_host.so")
    csrc = os.path.join(HERE, "..", "spliser_amd", "csrc")
    srcs = [os.path.join(HERE, "hostsim", "genecount_wave_host.cpp"), os.path.join(HERE, "hostsim", "wave_emul.h"), os.path.join(csrc, "spl_genecount_wave.h"),
            os.path.join(csrc, "spl_wave.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
    return ctypes.CDLL(so)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run(lib, results, n_genes):
    """-> (counts[n_genes], specials[3], the adds as a sorted list of (gene, value))."""
    results = np.ascontiguousarray(results, np.uint32)
    counts, specials = np.zeros(max(n_genes, 1), np.uint64), np.zeros(3, np.uint64)
    adds, n_adds = np.zeros(2 * max(len(results), 1), np.uint64), ctypes.c_uint64(0)
    rc = lib.genecount_wave_run(_ptr(results), ctypes.c_uint64(len(results)), ctypes.c_uint32(n_genes), _ptr(counts), _ptr(specials), _ptr(adds),
                                ctypes.c_uint64(len(adds) // 2), ctypes.byref(n_adds))
    assert rc == 0, "the wave broke a rule of the emulator (%d)" % rc
    pairs = adds[:2 * n_adds.value].reshape(-1, 2).tolist()
    return counts[:n_genes].tolist(), specials.tolist(), sorted((int(g), int(v)) for g, v in pairs)


def want(results, n_genes):
    """Plain loops: the counts, and one add per run of equal gene results within each 64 of them."""
    counts, specials, adds = [0] * n_genes, [0, 0, 0], []
    for i, r in enumerate(results):
        r = int(r)
        if r < n_genes:
            counts[r] += 1
            if i % 64 == 0 or int(results[i - 1]) != r:
                adds.append([r, 0])
                head = adds[-1]
            head[1] += 1
        elif NO_FEATURE <= r <= NOT_COUNTED:
            specials[r - NO_FEATURE] += 1
    return counts, specials, sorted((g, v) for g, v in adds)


def both(lib, results, n_genes):
    got = run(lib, results, n_genes)
    assert got == want(results, n_genes)
    return got


def test_sixty_four_equal_results_are_one_add_of_64(lib):
    counts, specials, adds = both(lib, [5] * 64, 9)
    assert adds == [(5, 64)] and counts[5] == 64 and specials == [0, 0, 0]


def test_sixty_four_different_results_are_64_adds(lib):
    counts, _, adds = both(lib, list(range(64)), 64)
    assert adds == [(g, 1) for g in range(64)] and counts == [1] * 64


@pytest.mark.parametrize("head", [1, 31, 32, 63])
def test_a_head_at_lane(lib, head):
    _, _, adds = both(lib, [3] * head + [4] * (64 - head), 6)
    assert adds == [(3, head), (4, 64 - head)]


def test_heads_at_lanes_1_31_32_and_63_together(lib):
    results = [0] + [1] * 30 + [2] + [3] * 31 + [4]
    _, _, adds = both(lib, results, 5)
    assert adds == [(0, 1), (1, 30), (2, 1), (3, 31), (4, 1)]


@pytest.mark.parametrize("n", [1, 2, 37, 63, 65, 130])
def test_a_wave_that_is_not_full(lib, n):
    """The lanes behind the last read are idle: they end the last run and are counted nowhere."""
    counts, specials, adds = both(lib, [2] * n, 3)
    assert counts == [0, 0, n] and specials == [0, 0, 0]
    assert adds == sorted((2, min(64, n - b)) for b in range(0, n, 64))


def test_results_that_return_to_an_earlier_value_are_three_adds(lib):
    a, b = 7, 2
    _, _, adds = both(lib, [a] * 10 + [b] * 5 + [a] * 49, 8)
    assert adds == [(2, 5), (7, 10), (7, 49)]


def test_special_results_cut_runs_and_are_counted_by_ballot(lib):
    results = [1] * 4 + [NO_FEATURE] * 3 + [1] * 2 + [AMBIGUOUS] + [NOT_COUNTED] * 5 + [0] * 49
    counts, specials, adds = both(lib, results, 2)
    assert specials == [3, 1, 5] and adds == [(0, 49), (1, 2), (1, 4)] and counts == [49, 6]
    _, specials, adds = both(lib, [NOT_COUNTED] * 64 + [NO_FEATURE] * 64 + [AMBIGUOUS] * 11, 2)
    assert specials == [64, 11, 64] and adds == []


def test_a_result_beyond_the_genes_is_counted_nowhere(lib):
    """There is none (the maps' codes are checked); said for the memory's sake."""
    counts, specials, adds = run(lib, [0, 1, 2, 2, 1], 2)
    assert counts == [1, 2] and specials == [0, 0, 0] and adds == [(0, 1), (1, 1), (1, 1)]


def test_random_results_over_many_waves_and_the_yardsticks_run_heads(lib):
    rng = np.random.default_rng(20261019)
    n_genes = 40
    for n, p_change in ((64 * 7 + 13, 0.05), (64 * 5, 0.5), (1000, 1.0)):
        results, cur = [], 0
        for _ in range(n):
            if rng.random() < p_change:
                cur = int(rng.choice([int(rng.integers(0, n_genes)), NO_FEATURE, AMBIGUOUS, NOT_COUNTED], p=[0.7, 0.1, 0.1, 0.1]))
            results.append(cur)
        counts, specials, adds = both(lib, results, n_genes)
        assert sum(counts) + sum(specials) == n
        as_yardstick = [r if r < n_genes else NO_FEATURE - r - 1 for r in results]       # genecases' results: -1, -2, -3
        assert len(adds) == G.run_heads(as_yardstick) and G.counts_of(as_yardstick, n_genes) == counts + specials
