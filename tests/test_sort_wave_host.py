"""The stable radix sort of ``--anyOrder`` (spliser_amd/csrc/spl_sort_wave.h: the bodies of spl_sort.hip's kernels) built for the
host against tests/hostsim/wave_emul.h -- a wave = 64 fibers, every cross-lane primitive a checked rendezvous -- and held against
numpy's stable sort.  The reference has no such step: its input is sorted by ``samtools sort`` before it is read
(SpliSER_v0_1_8.py:422 reads through ``samtools view BAM region``, which needs the index of a sorted file)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from ordercases import sort_cases

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_PARTS = 2048


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(HERE, "hostsim", "libsort_wave_host.so")
    csrc = os.path.join(HERE, "..", "spliser_amd", "csrc")
    srcs = [os.path.join(HERE, "hostsim", "sort_wave_host.cpp"), os.path.join(HERE, "hostsim", "wave_emul.h"), os.path.join(csrc, "spl_sort_wave.h"),
            os.path.join(csrc, "spl_wave.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
    L = ctypes.CDLL(so)
    L.sort_wave_tile.restype = ctypes.c_uint32
    L.sort_wave_parts.restype = ctypes.c_uint32
    L.sort_wave_passes.restype = ctypes.c_uint32
    return L


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def sort_keys(lib, keys, key_bits, max_parts=MAX_PARTS):
    keys = np.ascontiguousarray(keys, np.uint64)
    perm = np.full(max(len(keys), 1), 0xffffffff, np.uint32)
    rc = lib.sort_wave_keys(_ptr(keys), ctypes.c_uint64(len(keys)), ctypes.c_uint32(key_bits), ctypes.c_uint32(max_parts), _ptr(perm))
    assert rc == 0, "the wave broke a rule of the emulator (%d)" % rc
    return perm[:len(keys)]


def test_the_passes_of_a_key(lib):
    """Only the digits that can differ: the low word's (POS) from bit 0, the high word's (reference id) from bit 32."""
    sh = (ctypes.c_uint32 * 8)()
    want = {1: [0], 8: [0], 9: [0, 8], 32: [0, 8, 16, 24], 33: [0, 8, 16, 24, 32], 40: [0, 8, 16, 24, 32], 41: [0, 8, 16, 24, 32, 40],
            63: [0, 8, 16, 24, 32, 40, 48, 56], 64: [0, 8, 16, 24, 32, 40, 48, 56]}
    for bits, shifts in want.items():
        n = lib.sort_wave_passes(ctypes.c_uint32(bits), sh)
        assert list(sh[:n]) == shifts, bits


def test_one_pass_histogram_rank_and_scatter(lib):
    """One pass on three tiles and five keys, in four parts and in two (a part of two tiles): the histogram per part is numpy's
    bincount of the part's digits, and the scatter is the stable sort by that digit alone."""
    tile = lib.sort_wave_tile()
    rng = np.random.default_rng(5)
    n = 3 * tile + 5
    keys = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    perm_in = rng.permutation(n).astype(np.uint32)
    for max_parts, shift in ((MAX_PARTS, 0), (MAX_PARTS, 32), (2, 8), (1, 16)):
        parts = lib.sort_wave_parts(ctypes.c_uint64(n), ctypes.c_uint32(max_parts))
        assert parts == min(4, max_parts)
        per = -(-4 // parts) * tile
        keys_out, perm_out, hist = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(256 * parts, np.uint32)
        rc = lib.sort_wave_pass(_ptr(keys), _ptr(perm_in), ctypes.c_uint64(n), ctypes.c_uint32(shift), ctypes.c_uint32(max_parts), _ptr(keys_out), _ptr(perm_out), _ptr(hist))
        assert rc == 0
        digit = ((keys >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)
        for p in range(parts):
            assert np.array_equal(hist.reshape(256, parts)[:, p], np.bincount(digit[p * per:(p + 1) * per], minlength=256)), (max_parts, p)
        order = np.argsort(digit, kind="stable")
        assert np.array_equal(keys_out, keys[order]) and np.array_equal(perm_out, perm_in[order]), (max_parts, shift)


def test_the_whole_sort_against_numpy(lib):
    tile = lib.sort_wave_tile()
    for name, keys, bits in sort_cases(tile):
        got = sort_keys(lib, keys, bits)
        want = np.argsort(keys, kind="stable").astype(np.uint32)
        assert np.array_equal(got, want), name
        if name == "all equal":
            assert np.array_equal(got, np.arange(len(keys), dtype=np.uint32))


def test_parts_of_several_tiles(lib):
    """More tiles than parts -- a wave walks its tiles in order, the digits' offsets running on in its shared memory -- with
    long runs of equal keys across the tiles' and the parts' borders."""
    tile = lib.sort_wave_tile()
    rng = np.random.default_rng(9)
    n = 7 * tile + 13
    seven = rng.integers(0, 1 << 40, 7, dtype=np.uint64)
    for keys in (rng.integers(0, 1 << 40, n, dtype=np.uint64), seven[rng.integers(0, 7, n)]):
        for max_parts in (1, 2, 3):
            assert np.array_equal(sort_keys(lib, keys, 40, max_parts), np.argsort(keys, kind="stable").astype(np.uint32)), max_parts


def test_the_scan_of_the_gather(lib):
    """Inclusive prefix sums of 32-bit counts in place, in the same parts: what turns the op counts in their new order into cig_off."""
    tile = lib.sort_wave_tile()
    rng = np.random.default_rng(3)
    for n in (0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 5):
        for max_parts in (MAX_PARTS, 2):
            v = rng.integers(0, 9, max(n, 1), dtype=np.uint32)
            v[::7] = 0      # (reads without a CIGAR: empty runs)
            want = np.cumsum(v[:n], dtype=np.uint64).astype(np.uint32)
            rc = lib.sort_wave_scan(_ptr(v), ctypes.c_uint64(n), ctypes.c_uint32(max_parts))
            assert rc == 0
            assert np.array_equal(v[:n], want), (n, max_parts)
