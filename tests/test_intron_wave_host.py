"""How a team of lanes of ``spl_intron_depth`` takes the trimmed depth of one intron (spliser_amd/csrc/spl_intron_wave.h: the body
the kernels of spl_intron.hip call per intron) built for the host against tests/hostsim/wave_emul.h -- a wave = 64 fibers, every
cross-lane primitive a checked rendezvous -- and held against the yardstick's base-by-base expansion (introncases.py): the searches
for a piece's boundaries, the stretches, the radix selection of both rank values and the sum.  The reference has no such step."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import introncases as I

HERE = os.path.dirname(os.path.abspath(__file__))
TRIMS = (0, 30, 49)


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(HERE, "hostsim", "libintron_wave_host.so")
    csrc = os.path.join(HERE, "..", "spliser_amd", "csrc")
    srcs = [os.path.join(HERE, "hostsim", "intron_wave_host.cpp"), os.path.join(HERE, "hostsim", "wave_emul.h"), os.path.join(csrc, "spl_intron_wave.h"), os.path.join(csrc, "spl_wave.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
    return ctypes.CDLL(so)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run(lib, pos, depth, introns, trim):
    """introns: [[(ps, pe)]] -> [(L, covered, depth_n, depth_sum)]."""
    pos, depth = np.asarray(list(pos) + [0], np.int32), np.asarray(list(depth) + [0], np.uint32)
    off = np.zeros(len(introns) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in introns])
    start = np.asarray([p[0] for pieces in introns for p in pieces] + [0], np.int32)
    end = np.asarray([p[1] for pieces in introns for p in pieces] + [0], np.int32)
    out = np.full((len(introns), 4), -1, np.int64)
    rc = lib.intron_wave_run(_ptr(pos), _ptr(depth), ctypes.c_int64(len(pos) - 1), ctypes.c_int64(len(introns)), _ptr(off), _ptr(start), _ptr(end), ctypes.c_uint32(trim), _ptr(out))
    assert rc == 0, "the wave broke a rule of the emulator (%d)" % rc
    return [tuple(r) for r in out.tolist()]


def both(lib, pos, depth, introns, length, trims=TRIMS):
    per_base = I.depth_per_base(pos, depth, length)
    got = None
    for trim in trims:
        got = run(lib, pos, depth, introns, trim)
        assert got == [I.stats_of(per_base, pieces, trim) for pieces in introns], "trim %d" % trim
    return got


CASES = I.body_cases()


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c[0] for c in CASES])
def test_body_cases(lib, k):
    """The cases the kernel's tests run on the device too."""
    _, pos, depth, introns, length = CASES[k]
    both(lib, pos, depth, introns, length)


def test_a_piece_with_no_boundary_inside(lib):
    """At depth 0 -- before every boundary, and behind a boundary that says 0 -- and at a depth above 0."""
    got = both(lib, [50, 90, 200], [9, 0, 4], [[(10, 40)], [(100, 150)], [(55, 80)], [(300, 1000)]], 1000, trims=(30,))
    assert got == [(30, 0, 12, 0), (50, 0, 20, 0), (25, 25, 11, 99), (700, 700, 280, 1120)]
    assert both(lib, [], [], [[(0, 10)], [(5, 6), (8, 20)]], 20, trims=(0,)) == [(10, 0, 10, 0), (13, 0, 13, 0)]


def test_a_piece_that_starts_or_ends_exactly_on_a_boundary(lib):
    pos, depth = [100, 110, 120, 130], [1, 2, 3, 0]
    got = both(lib, pos, depth, [[(100, 110)], [(110, 130)], [(105, 120)], [(90, 100)], [(120, 121)], [(129, 131)], [(130, 140)]], 200, trims=(0,))
    assert got == [(10, 10, 10, 10), (20, 20, 20, 50), (15, 15, 15, 25), (10, 0, 10, 0), (1, 1, 1, 3), (2, 1, 2, 3), (10, 0, 10, 0)]


def test_both_ranks_on_one_value_and_in_different_buckets(lib):
    # 100 bases: 10 of depth 1, 80 of depth 5, 10 of depth 70000 -- trim 30 and 49 have both ranks on 5, trim 0 has 1 and 70000
    pos, depth = [0, 10, 90], [1, 5, 70000]
    got = {trim: both(lib, pos, depth, [[(0, 100)]], 100, trims=(trim,))[0] for trim in TRIMS}
    assert got[0] == (100, 100, 100, 10 + 400 + 700000) and got[30] == (100, 100, 40, 200) and got[49] == (100, 100, 2, 10)
    # ties that straddle lo and hi: 3 x 2, 4 x 9, 3 x 300; trim 30 of 10 bases: D[3:7] = 9 9 9 9; trim 20: D[2:8] = 2 9 9 9 9 300
    pos, depth = [0, 3, 7], [2, 9, 300]
    assert both(lib, pos, depth, [[(0, 10)]], 10, trims=(30,))[0] == (10, 10, 4, 36)
    assert both(lib, pos, depth, [[(0, 10)]], 10, trims=(20,))[0] == (10, 10, 6, 2 + 36 + 300)
    # the two values in different buckets of the TOP byte, something between them
    pos, depth = [0, 2, 4, 6], [5, 0x02000000, 0x10000007, 0xF0000000]
    assert both(lib, pos, depth, [[(0, 8)]], 8, trims=(25,))[0] == (8, 8, 4, 2 * 0x02000000 + 2 * 0x10000007)


def test_the_greatest_depth(lib):
    top = 2 ** 32 - 1
    assert both(lib, [0, 10], [top, 0], [[(0, 10)], [(5, 20)]], 20, trims=(0,)) == [(10, 10, 10, 10 * top), (15, 5, 15, 5 * top)]


def test_random_introns(lib):
    rng = np.random.default_rng(20261020)
    for n_bound, max_depth in ((0, 1), (1, 3), (30, 3), (300, 40), (300, 2 ** 32 - 1)):
        length = 700
        pos, depth = I.random_bounds(rng, length, n_bound, max_depth)
        introns = [I.random_pieces(rng, length, int(rng.integers(1, 8))) for _ in range(25)] + [[(0, length)]]
        both(lib, pos, depth, introns, length)
