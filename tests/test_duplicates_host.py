"""Duplicate marking without a GPU: the rule header behind a stable sort on the host (``spl_duplicates_host``) against its
restatement in Python integers (``dupcases.py``) on every case, marks, counters and histogram; the mask compaction's tile body
(spliser_amd/csrc/spl_dups_wave.h over spl_subsample_wave.h) under the wave emulator against numpy's boolean mask; and the rule
header alone under AddressSanitizer and UBSan in a program of its own (tests/hostsim/dup_rule_asan.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dupcases as D
import matecases as M
import subsamplecases as S
from spliser_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


@pytest.fixture(scope="module")
def cases(built):
    return D.all_cases(native.subsample_tile())


def _arrays(rs):
    return native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)


# ---- the rule -----------------------------------------------------------------------------------------------------------------
def test_the_cases_cover_what_the_issue_lists(cases):
    D.assert_covers(cases, native.subsample_tile())
    assert native.DUP_COUNTS == D.COUNTS and native.DUP_HIST == D.HIST


def test_the_unclipped_end_by_the_issues_numbers():
    ops = lambda text: D.G.ops(text).tolist()
    assert D.end_of(1, 0, ops("5S20M")) == (-4, 0)
    assert D.end_of(100, 0, ops("2H3S20M4S1H")) == (95, 0)
    assert D.end_of(100, 16, ops("2H3S20M4S1H")) == (100 + 20 - 1 + 5, 1)
    assert D.end_of(100, 16, ops("10M5D3I10N10M2=1X")) == (100 + 38 - 1, 1)
    assert D.end_of(100, 0, ops("10S5H")) == (85, 0) and D.end_of(100, 16, ops("10S5H")) == (99, 1)
    assert D.end_of(2 ** 31 - 1, 16, [(2 ** 28 - 1) << 4]) == (2 ** 31 - 1, 1)          # clamped
    assert D.end_of(1, 0, [(2 ** 28 - 1) << 4 | 4] * 9) == (-2 ** 31, 0)


def test_the_host_hook_against_the_restatement(cases):
    for name, segs in cases:
        for k, rs in enumerate(segs):
            mate, _ = native.mate_table_host(_arrays(rs), rs.keys)
            want_mate, _ = M.mate_table_of(rs, rs.keys.tolist())
            assert mate.tolist() == want_mate, (name, k)
            dup, counts, hist = native.duplicates_host(_arrays(rs), rs.keys, mate)
            want = D.duplicates(rs, rs.keys.tolist(), want_mate)
            assert np.array_equal(dup, want[0]), (name, k)
            assert counts == want[1], (name, k)
            assert np.array_equal(hist, want[2]), (name, k)


def test_the_host_hook_at_the_ends_of_the_coordinate_space(built):
    """Ends beyond 32 bits are clamped, not wrapped: two reads whose ends differ only beyond the clamp are one group."""
    seg = D.Segment(np.random.default_rng(1))
    big = (2 ** 28 - 1) << 4
    seg.read(16, 2 ** 30, [big] * 8, 10); seg.read(16, 2 ** 30, [big] * 9, 12); seg.read(0, 1, [big | 4] * 9 + [5 << 4], 14); seg.read(0, 1, [big | 4] * 10 + [5 << 4], 16)
    rs = seg.reads()
    mate = np.full(rs.n, M.NONE, np.uint32)
    dup, counts, hist = native.duplicates_host(_arrays(rs), rs.keys, mate)
    want = D.duplicates(rs, rs.keys.tolist(), mate.tolist())
    assert np.array_equal(dup, want[0]) and counts == want[1] and int(dup.sum()) == 2


def test_a_foreign_mate_table_reads_nothing_beyond_the_segment(built):
    rs = D.crowd(np.random.default_rng(2), 50)
    mate = np.full(rs.n, 5000, np.uint32)          # (no read of this segment: no mate)
    dup, counts, _ = native.duplicates_host(_arrays(rs), rs.keys, mate)
    want = D.duplicates(rs, rs.keys.tolist(), [M.NONE] * rs.n)
    assert np.array_equal(dup, want[0]) and counts == want[1]


# ---- the mask compaction's tile body under the wave emulator --------------------------------------------------------------------
@pytest.fixture(scope="module")
def wave():
    so = os.path.join(HERE, "hostsim", "libdups_wave_host.so")
    csrc = os.path.join(ROOT, "spliser_amd", "csrc")
    srcs = [os.path.join(HERE, "hostsim", "dups_wave_host.cpp"), os.path.join(HERE, "hostsim", "wave_emul.h")] + [
        os.path.join(csrc, h) for h in ("spl_dups_wave.h", "spl_subsample_wave.h", "spl_subsample.h", "spl_subsample_rule.h", "spl_read_view.h", "spl_wave.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
    L = ctypes.CDLL(so)
    L.dups_wave_tile.restype = ctypes.c_uint32
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _check_wave(L, name, segs, masks, with_strand):
    """The segments laid end to end with a few foreign entries in front of each, whose bytes say "kept" and "dropped": what a
    set does not cover is not looked at."""
    pad = S.reads_of(["once", "none"], np.array([1, 2], np.uint64), np.random.default_rng(0))
    parts, marks, first, at = [], [], [], 0
    for rs, mask in zip(segs, masks):
        parts += [pad, rs]
        marks += [np.array([0, 1], np.uint8), (~np.asarray(mask, bool)).astype(np.uint8) * np.uint8(1 + at % 200)]      # (any byte that is not 0 drops)
        first.append(at + pad.n)
        at += pad.n + rs.n
    cat = lambda f, dt: np.ascontiguousarray(np.concatenate([f(p) for p in parts]), dt)
    pos, flag, xs, keys = cat(lambda p: p.pos, np.int32), cat(lambda p: p.flag, np.uint16), cat(lambda p: p.xs, np.uint8), cat(lambda p: p.keys, np.uint64)
    cigar, dup = cat(lambda p: p.cigar, np.uint32), np.ascontiguousarray(np.concatenate(marks), np.uint8)
    off = np.concatenate(([0], np.cumsum(np.concatenate([p.n_ops for p in parts])))).astype(np.uint32)
    n, n_ops = len(pos), len(cigar)
    seg_first, seg_n = np.array(first, np.int64), np.array([rs.n for rs in segs], np.int64)
    out = dict(pos=np.full(n + 1, -7, np.int32), flag=np.full(n + 1, 0xdddd, np.uint16), cig_off=np.full(n + 2, 0xdddddddd, np.uint32), cigar=np.full(n_ops + 1, 0xdddddddd, np.uint32),
               xs=np.full(n + 1, 0xdd, np.uint8) if with_strand else None, keys=np.full(n + 1, 0xdddd, np.uint64), index=np.full(n + 1, 0xdddddddd, np.uint32))
    kept = np.zeros(2 * max(len(segs), 1), np.int64)
    rc = L.dups_wave_run(ctypes.c_uint32(len(segs)), _ptr(seg_first), _ptr(seg_n), ctypes.c_int64(n), ctypes.c_int64(n_ops), _ptr(pos), _ptr(flag), _ptr(off), _ptr(cigar),
                         _ptr(xs) if with_strand else None, _ptr(keys), _ptr(dup), ctypes.c_int64(n), ctypes.c_int64(n_ops), _ptr(out["pos"]), _ptr(out["flag"]),
                         _ptr(out["cig_off"]), _ptr(out["cigar"]), _ptr(out["xs"]), _ptr(out["keys"]), _ptr(out["index"]), _ptr(kept))
    assert rc == 0, "the wave broke a rule of the emulator (%d)" % rc
    kept, kept_ops = kept[:len(segs)], kept[len(segs):2 * len(segs)]
    want = [rs.masked(m) for rs, m in zip(segs, masks)]
    assert kept.tolist() == [w.n for w in want], name
    assert kept_ops.tolist() == [len(w.cigar) for w in want], name
    n_kept, n_kept_ops = int(kept.sum()), int(kept_ops.sum())
    cat = lambda f: np.concatenate([f(w) for w in want]) if want else np.zeros(0)
    assert np.array_equal(out["pos"][:n_kept], cat(lambda w: w.pos)) and np.array_equal(out["flag"][:n_kept], cat(lambda w: w.flag)), name
    assert np.array_equal(out["keys"][:n_kept], cat(lambda w: w.keys)), name
    if with_strand:
        assert np.array_equal(out["xs"][:n_kept], cat(lambda w: w.xs)) and out["xs"][n_kept] == 0xdd, name
    assert np.array_equal(out["cigar"][:n_kept_ops], cat(lambda w: w.cigar)) and out["cigar"][n_kept_ops] == 0xdddddddd, name
    assert np.array_equal(out["cig_off"][:n_kept + 1], np.concatenate(([0], np.cumsum(cat(lambda w: w.n_ops))))), name
    base = np.concatenate(([0], np.cumsum([rs.n for rs in segs])))
    index = np.concatenate([base[k] + np.flatnonzero(m) for k, m in enumerate(masks)]) if masks else np.zeros(0)
    assert np.array_equal(out["index"][:n_kept], index), name
    assert out["pos"][n_kept] == -7 and out["flag"][n_kept] == 0xdddd and out["keys"][n_kept] == 0xdddd and out["cig_off"][n_kept + 1] == 0xdddddddd \
        and out["index"][n_kept] == 0xdddddddd, name


def test_the_tile_body_against_numpy_on_the_rules_marks(wave, cases):
    assert wave.dups_wave_tile() == native.subsample_tile()
    for k, (name, segs) in enumerate(cases):
        masks = [~D.duplicates(rs, rs.keys.tolist())[0] for rs in segs]
        _check_wave(wave, name, segs, masks, with_strand=k % 2 == 0)


def test_the_tile_body_against_numpy_on_any_mask(wave):
    """... and on the subsampling tests' shapes under their patterns: all, none, the ends, runs across a tile's edge, long CIGARs
    kept and dropped at a tile's edge."""
    tile = wave.dups_wave_tile()
    for k, (name, segs, seed, threshold) in enumerate(S.all_cases(tile)):
        _check_wave(wave, name, segs, [rs.mask(seed, threshold) for rs in segs], with_strand=k % 2 == 1)


# ---- the rule header under the sanitizers -------------------------------------------------------------------------------------
def test_header_under_the_sanitizers(tmp_path, cases):
    """The rule's header alone in a program of its own: every array in a heap block of exactly its size."""
    exe = str(tmp_path / "dup_rule_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostsim", "dup_rule_asan.cpp"), "-o", exe])
    text_of = lambda v: " ".join(str(int(x)) for x in v)
    lines, want = [], []
    for name, segs in cases:
        for rs in segs:
            if (rs.pos < 0).any():
                continue          # (the text carries no sign)
            keys = rs.keys.tolist()
            mate = M.mate_table_of(rs, keys)[0]
            lines.append("|".join([text_of(rs.pos), text_of(rs.flag), text_of(rs.cig_off), text_of(rs.cigar), text_of(keys), text_of(mate)]))
            frags, _ = D.fragments_of(rs, keys, mate)
            groups = {}
            for f in frags:
                groups[f[:2]] = groups.get(f[:2], 0) + 1
            want.append((["%d:%d:%d:%d" % (f[3], f[0], f[1], f[2]) for f in frags], D.duplicates(rs, keys, mate)[0].astype(int).tolist(), [groups[g] for g in sorted(groups)]))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stderr[-4000:]
    got = out.stdout.split("\n")
    assert len(got) >= 2 * len(want)
    for k, (sigs, marks, sizes) in enumerate(want):
        assert got[2 * k].split() == sigs, k
        left, _, right = got[2 * k + 1].partition("|")
        assert [int(v) for v in left.split()] == marks, k
        assert [int(v) for v in right.split()] == sizes, k
