"""Subsampling without a GPU: the rule header on the host (``spl_subsample_keep_host``) against its restatement in Python integers
(``subsamplecases.py``), the properties that follow from it (nested, one decision a name, the kept share), the tile body of
``spl_reads_subsample``'s kernels (spliser_amd/csrc/spl_subsample_wave.h) under the wave emulator against numpy's boolean mask on
the GPU test's cases, and the rule header alone under AddressSanitizer and UBSan (tests/hostsim/subsample_rule_asan.cpp)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import matecases as M
import subsamplecases as S
from spliser_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


def _random_reads(rng, n):
    keys = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    keys[::11] = 0
    pos = rng.integers(-5, 2 ** 31 - 1, n).astype(np.int32)
    flag = rng.integers(0, 65536, n).astype(np.uint16)
    n_ops = rng.integers(0, 70000, n)
    n_ops[::5] = rng.integers(0, 4, len(n_ops[::5]))
    return keys, pos, flag, np.concatenate(([0], np.cumsum(n_ops))).astype(np.uint32)


# ---- the rule -----------------------------------------------------------------------------------------------------------------
def test_the_hook_against_the_restatement(built):
    rng = np.random.default_rng(1)
    keys, pos, flag, off = _random_reads(rng, 3000)
    n_ops = np.diff(off.astype(np.int64))
    seeds = [0, 1, 7, 12345, 2 ** 64 - 1, int(rng.integers(0, 2 ** 63))]
    for seed in seeds:
        for threshold in (0, 1, S.ALL // 20, S.ALL // 2, S.ALL - 1, S.ALL, int(rng.integers(0, S.ALL))):
            got = native.subsample_keep_host(keys, pos, flag, off, seed, threshold)
            assert np.array_equal(got, S.keep_mask(keys, pos, flag, n_ops, seed, threshold)), (seed, threshold)
            if threshold == 0:
                assert not got.any()
            if threshold == S.ALL:
                assert got.all()
    with pytest.raises(native.SpliserNativeError, match="2\\^32"):
        native.subsample_keep_host(keys, pos, flag, off, 0, S.ALL + 1)


def test_the_recipe_by_the_issues_numbers():
    """The recipe once more, step by step on one key, against the yardstick."""
    key, seed = 0x0123456789abcdef, 7
    z = key ^ ((seed * 0x9e3779b97f4a7c15) % 2 ** 64)
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) % 2 ** 64
    z ^= z >> 31
    assert S.draw(key, seed) == z >> 32
    assert S.thresholds(4) == [2 ** 30, 2 ** 31, 3 * 2 ** 30, 2 ** 32]


def test_reads_without_a_name_fall_back_to_pos_flag_and_ops(built):
    rng = np.random.default_rng(2)
    _, pos, flag, off = _random_reads(rng, 2000)
    n_ops = np.diff(off.astype(np.int64))
    stand_in = np.array([S.nameless_key(int(p), int(f), int(o)) for p, f, o in zip(pos, flag, n_ops)], np.uint64)
    assert (stand_in != 0).all()
    zero = np.zeros(2000, np.uint64)
    for seed, threshold in ((0, S.ALL // 2), (9, S.ALL // 3)):
        nameless = native.subsample_keep_host(zero, pos, flag, off, seed, threshold)
        named = native.subsample_keep_host(stand_in, np.zeros(2000, np.int32), np.zeros(2000, np.uint16), np.zeros(2001, np.uint32), seed, threshold)
        assert np.array_equal(nameless, named) and 0 < nameless.sum() < 2000
    # ... and only the low 16 bits of the op count count
    a = native.subsample_keep_host(zero[:1], [77], [99], [0, 3], 1, S.ALL // 2)
    b = native.subsample_keep_host(zero[:1], [77], [99], [0, 3 + 65536], 1, S.ALL // 2)
    assert a.tolist() == b.tolist()


def test_nested_over_twenty_thresholds(built):
    rng = np.random.default_rng(3)
    keys, pos, flag, off = _random_reads(rng, 5000)
    for seed in (0, 4):
        before = np.zeros(5000, bool)
        for threshold in S.thresholds(20):
            now = native.subsample_keep_host(keys, pos, flag, off, seed, threshold)
            assert not (before & ~now).any() and now.sum() >= before.sum()
            before = now
        assert before.all()


def test_two_records_of_one_name_share_a_decision(built):
    rng = np.random.default_rng(4)
    names = [b"frag.%d" % k for k in range(1500)]
    keys = np.array([M.name_key(n) for n in names] * 3, np.uint64)        # mates, and a supplementary record
    _, pos, flag, off = _random_reads(rng, 4500)
    for seed in (0, 1, 99):
        got = native.subsample_keep_host(keys, pos, flag, off, seed, S.ALL // 2)
        assert np.array_equal(got[:1500], got[1500:3000]) and np.array_equal(got[:1500], got[3000:])
        assert 0 < got[:1500].sum() < 1500


def test_the_kept_share_of_twenty_thousand_names(built):
    """Within 5 standard deviations of f * N, a binomial's: a condition, not a measurement."""
    n = 20000
    zeros, off = np.zeros(n, np.int32), np.zeros(n + 1, np.uint32)
    for shape in ("r%06d", "frag.%d", "SRR1.%d/1"):
        keys = np.array([M.name_key((shape % k).encode()) for k in range(n)], np.uint64)
        for seed in (0, 1, 7, 12345):
            for k in range(1, 20):
                f = k / 20.0
                kept = int(native.subsample_keep_host(keys, zeros, zeros.astype(np.uint16), off, seed, (k << 32) // 20).sum())
                assert abs(kept - f * n) <= 5 * math.sqrt(n * f * (1 - f)), (shape, seed, k, kept)


def test_keys_for_a_pattern_give_that_pattern():
    rng = np.random.default_rng(6)
    pattern = rng.random(500) < 0.3
    keys = S.keys_for(pattern, 5, S.ALL // 2)
    assert len(set(keys.tolist())) == 500 and int(keys.max()) < 5000
    assert np.array_equal(S.keep_mask(keys, np.zeros(500), np.zeros(500), np.zeros(500), 5, S.ALL // 2), pattern)


# ---- the tile body under the wave emulator ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wave():
    so = os.path.join(HERE, "hostsim", "libsubsample_wave_host.so")
    csrc = os.path.join(ROOT, "spliser_amd", "csrc")
    srcs = [os.path.join(HERE, "hostsim", "subsample_wave_host.cpp"), os.path.join(HERE, "hostsim", "wave_emul.h")] + [
        os.path.join(csrc, h) for h in ("spl_subsample_wave.h", "spl_subsample.h", "spl_subsample_rule.h", "spl_read_view.h", "spl_wave.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
    L = ctypes.CDLL(so)
    L.subsample_wave_tile.restype = ctypes.c_uint32
    L.subsample_wave_lane_ops.restype = ctypes.c_uint32
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _run_wave(L, segs, seed, threshold, with_strand):
    """The segments laid end to end with a few foreign entries in front of each (a set need not cover its arrays) -> the selected
    arrays, the index and the kept reads per segment."""
    pad = S.reads_of(["once", "none"], np.array([1, 2], np.uint64), np.random.default_rng(0))
    parts, first, at = [], [], 0
    for rs in segs:
        parts += [pad, rs]
        first.append(at + pad.n)
        at += pad.n + rs.n
    cat = lambda f, dt: np.ascontiguousarray(np.concatenate([f(p) for p in parts]), dt)
    pos, flag, xs, keys = cat(lambda p: p.pos, np.int32), cat(lambda p: p.flag, np.uint16), cat(lambda p: p.xs, np.uint8), cat(lambda p: p.keys, np.uint64)
    cigar = cat(lambda p: p.cigar, np.uint32)
    off = np.concatenate(([0], np.cumsum(np.concatenate([p.n_ops for p in parts])))).astype(np.uint32)
    n, n_ops = len(pos), len(cigar)
    seg_first, seg_n = np.array(first, np.int64), np.array([rs.n for rs in segs], np.int64)
    out = dict(pos=np.full(n + 1, -7, np.int32), flag=np.full(n + 1, 0xdddd, np.uint16), cig_off=np.full(n + 2, 0xdddddddd, np.uint32), cigar=np.full(n_ops + 1, 0xdddddddd, np.uint32),
               xs=np.full(n + 1, 0xdd, np.uint8) if with_strand else None, keys=np.full(n + 1, 0xdddd, np.uint64), index=np.full(n + 1, 0xdddddddd, np.uint32))
    kept = np.zeros(2 * max(len(segs), 1), np.int64)
    rc = L.subsample_wave_run(ctypes.c_uint32(len(segs)), _ptr(seg_first), _ptr(seg_n), ctypes.c_int64(n), ctypes.c_int64(n_ops), _ptr(pos), _ptr(flag), _ptr(off), _ptr(cigar),
                              _ptr(xs) if with_strand else None, _ptr(keys), ctypes.c_uint64(seed), ctypes.c_uint64(threshold), ctypes.c_int64(n), ctypes.c_int64(n_ops),
                              _ptr(out["pos"]), _ptr(out["flag"]), _ptr(out["cig_off"]), _ptr(out["cigar"]), _ptr(out["xs"]), _ptr(out["keys"]), _ptr(out["index"]), _ptr(kept))
    assert rc == 0, "the wave broke a rule of the emulator (%d)" % rc
    return out, kept[:len(segs)], kept[len(segs):2 * len(segs)]


def _check_wave(L, name, segs, seed, threshold, with_strand):
    out, kept, kept_ops = _run_wave(L, segs, seed, threshold, with_strand)
    masks = [rs.mask(seed, threshold) for rs in segs]
    want = [rs.masked(m) for rs, m in zip(segs, masks)]
    assert kept.tolist() == [w.n for w in want], name
    assert kept_ops.tolist() == [len(w.cigar) for w in want], name
    n, n_ops = int(kept.sum()), int(kept_ops.sum())
    cat = lambda f: np.concatenate([f(w) for w in want]) if want else np.zeros(0)
    assert np.array_equal(out["pos"][:n], cat(lambda w: w.pos)) and np.array_equal(out["flag"][:n], cat(lambda w: w.flag)), name
    assert np.array_equal(out["keys"][:n], cat(lambda w: w.keys)), name
    if with_strand:
        assert np.array_equal(out["xs"][:n], cat(lambda w: w.xs)) and out["xs"][n] == 0xdd, name
    assert np.array_equal(out["cigar"][:n_ops], cat(lambda w: w.cigar)) and out["cigar"][n_ops] == 0xdddddddd, name
    assert np.array_equal(out["cig_off"][:n + 1], np.concatenate(([0], np.cumsum(cat(lambda w: w.n_ops))))), name
    base = np.concatenate(([0], np.cumsum([rs.n for rs in segs])))
    index = np.concatenate([base[k] + np.flatnonzero(m) for k, m in enumerate(masks)]) if masks else np.zeros(0)
    assert np.array_equal(out["index"][:n], index), name
    # nothing beyond what was kept is written
    assert out["pos"][n] == -7 and out["flag"][n] == 0xdddd and out["keys"][n] == 0xdddd and out["cig_off"][n + 1] == 0xdddddddd and out["index"][n] == 0xdddddddd, name


def test_the_tile_body_against_numpy(wave):
    tile = wave.subsample_wave_tile()
    assert tile % 64 == 0 and wave.subsample_wave_lane_ops() < 9          # (the cases' long CIGARs are longer than a lane copies)
    cases = S.all_cases(tile)
    assert len(cases) > 60
    for k, (name, segs, seed, threshold) in enumerate(cases):
        _check_wave(wave, name, segs, seed, threshold, with_strand=k % 2 == 0)
    for name, segs, seed, threshold in S.cigar_cases(tile) + S.segment_cases(tile):
        _check_wave(wave, name, segs, seed, threshold, with_strand=True)
        _check_wave(wave, name, segs, seed, threshold, with_strand=False)


def test_the_tile_body_at_the_thresholds_ends_and_twice_over(wave):
    tile = wave.subsample_wave_tile()
    rng = np.random.default_rng(8)
    n = tile + 30
    rs = S.reads_of(S.mixed_kinds(n, rng), rng.integers(0, 2 ** 63, n, dtype=np.uint64), rng)
    for threshold in (0, S.ALL):
        _check_wave(wave, "threshold %d" % threshold, [rs], 3, threshold, True)
    # a selection of a selection is the smaller selection
    t1, t2 = S.ALL // 4, (3 * S.ALL) // 4
    once = rs.masked(rs.mask(3, t2))
    twice = once.masked(once.mask(3, t1))
    direct = rs.masked(rs.mask(3, t1))
    assert np.array_equal(twice.keys, direct.keys) and np.array_equal(twice.cigar, direct.cigar)
    _check_wave(wave, "twice", [once], 3, t1, True)


# ---- the rule header under the sanitizers -------------------------------------------------------------------------------------
def test_header_under_the_sanitizers(tmp_path):
    """The rule's header alone in a program of its own: every array in a heap block of exactly its size."""
    exe = str(tmp_path / "subsample_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostsim", "subsample_rule_asan.cpp"), "-o", exe])
    text_of = lambda v: " ".join(str(int(x)) for x in v)
    rng = np.random.default_rng(10)
    lines, want = [], []
    for seed, threshold in ((0, S.ALL // 2), (2 ** 64 - 1, S.ALL - 1), (7, 0), (7, S.ALL), (12345, 1)):
        keys, pos, flag, off = _random_reads(rng, 400)
        pos = np.abs(pos)          # (the text carries no sign; a negative POS is the hook's test)
        lines.append("|".join(["%d %d" % (seed, threshold), text_of(keys), text_of(pos), text_of(flag), text_of(off)]))
        want.append(S.keep_mask(keys, pos, flag, np.diff(off.astype(np.int64)), seed, threshold).astype(int).tolist())
    lines.append("3 5||||0")
    want.append([])
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stderr
    got = out.stdout.split("\n")
    assert len(got) >= len(want)
    for k, w in enumerate(want):
        assert [int(v) for v in got[k].split()] == w, k
