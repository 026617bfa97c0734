"""The two join kernels of compressed SAM and the order kernel of spl_sam.hip, launched one by one through ctypes on torch buffers with
guard bytes behind every output, as tests/test_gpu_sam_kernels.py launches the others: ``spl_sam_last_newline_kernel`` against
``bytes.rfind`` -- at both ends of [lo, hi), at every residue of lo and hi modulo 16, on a text long enough for its loop's second trip
and at offsets above 2^32 --, ``spl_sam_long_line_kernel`` against a plain walk of the line lengths, and ``spl_sam_order_kernel`` with
``first > 0``, where it must compare record ``first`` with the one in front of it.  Everything is exact.  The reference has no
counterpart: it reads what ``samtools view`` prints, line by line (SpliSER_v0_1_8.py:422)."""
import ctypes

import numpy as np
import pytest

import gathercases as G
import samcases as S
from test_gpu_sam_kernels import COUNTS, _dev, _host, _p, lib, window  # noqa: F401  (lib: the fixture)
from test_gpu_sort_gather import NULL, _inout

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ONE_TRIP = G.NEWLINE_ONE_TRIP                 # 8 MiB: the text that one trip of last_newline's loop takes
NO_LINE = 0xFFFFFFFF


def text_with(n, newlines, fill=b"x"):
    a = np.frombuffer(fill * n, np.uint8).copy()
    a[list(newlines)] = 10
    return a.tobytes()


def want_last(text, lo, hi):
    return text.rfind(b"\n", lo, hi) + 1


def last_newline(lib, text, lo, hi):
    buf, ptr = window(text, lo, hi)
    d_last, _ = _inout(np.zeros(1, np.uint64))          # (*last = 0: the caller's)
    assert lib.spl_dev_launch_sam_last_newline(ptr, ctypes.c_uint64(lo), ctypes.c_uint64(hi), _p(d_last), NULL) == 0
    torch.cuda.synchronize()
    del buf
    return int(_host(d_last, 8, np.uint64, "last")[0])


# ---- last_newline -------------------------------------------------------------------------------------------------------------------

def test_last_newline_at_the_ends_of_the_range(lib):
    lo, hi = 37, 70
    for title, newlines, want in (("at lo", [lo], lo + 1), ("at lo - 1 only", [lo - 1], 0), ("at hi - 1", [hi - 1], hi), ("at hi only", [hi], 0),
                                  ("at lo - 1 and at hi", [lo - 1, hi], 0), ("at lo and at hi - 1", [lo, hi - 1], hi), ("in front of hi - 1 and behind", [50, 61, hi, hi + 1], 62),
                                  ("none at all", [], 0)):
        text = text_with(100, newlines)
        assert want_last(text, lo, hi) == want, title
        assert last_newline(lib, text, lo, hi) == want, title
    assert last_newline(lib, text_with(5000, []), 3, 4990) == 0
    # lo and hi inside one 16-byte word, newlines on both sides of the range and none inside; then one inside
    lo, hi = 35, 41
    assert lo >> 4 == (hi - 1) >> 4
    assert last_newline(lib, text_with(100, [32, 33, 34, 41, 42, 47]), lo, hi) == 0
    assert last_newline(lib, text_with(100, [32, 33, 34, 38, 41, 42, 47]), lo, hi) == 39
    # a range of one byte
    for lo in (16, 21, 31):
        assert last_newline(lib, text_with(64, [lo]), lo, lo + 1) == lo + 1
        assert last_newline(lib, text_with(64, [lo - 1, lo + 1]), lo, lo + 1) == 0
    # an empty range launches nothing
    assert last_newline(lib, text_with(64, [20]), 20, 20) == 0


def test_last_newline_at_every_residue_of_lo_and_hi(lib):
    """16 x 16 ranges, lo and hi at every residue modulo 16, on two texts -- one with a newline in most words, one with three, of
    which two lie just outside most ranges --, every answer in a slot of its own."""
    rng = np.random.default_rng(14)
    a = rng.integers(97, 123, 128, dtype=np.uint8)
    a[rng.random(128) < 0.15] = 10
    texts = (a.tobytes(), text_with(128, [47, 70, 111]))
    d_last, _ = _inout(np.zeros(512, np.uint64))
    want, keep = [], []
    for text in texts:
        buf, ptr = window(text, 0, len(text))
        keep.append(buf)
        for r_lo in range(16):
            for r_hi in range(16):
                lo = 48 + r_lo
                hi = 64 + 16 * (r_lo % 3) + r_hi         # (one to four words; with r_hi = 0 and r_lo % 3 = 0 the range lies inside one)
                assert lo < hi <= 111 and lo % 16 == r_lo and hi % 16 == r_hi
                slot = ctypes.c_void_p(d_last.data_ptr() + 8 * len(want))
                assert lib.spl_dev_launch_sam_last_newline(ptr, ctypes.c_uint64(lo), ctypes.c_uint64(hi), slot, NULL) == 0
                want.append(want_last(text, lo, hi))
    torch.cuda.synchronize()
    got = _host(d_last, 8 * 512, np.uint64, "last").tolist()
    assert got == want
    assert sum(1 for w in want if w == 0) >= 40 and len(set(want)) >= 10        # (ranges without a newline, and many different answers)
    del keep


def test_last_newline_on_the_loops_second_trip(lib):
    """8 MiB + 4 KiB: the first 256 lanes take a second word, 8 MiB behind their first."""
    n = G.NEWLINE_TEXT
    assert G.newline_trips(0, n) == (2, 1) and G.newline_trips(3, n - 7) == (2, 1)
    behind = ONE_TRIP + 16 * 5 + 7            # (the second word of the lane that has byte 83 in its first)
    for title, newlines in (("its only newline in a first word of a lane that goes on to a second", [83]), ("... and in that lane's second word too", [83, behind]),
                            ("its only newline in the first 8 MiB, in a lane of one word", [ONE_TRIP - 3000]), ("its last newline in the tail", [12345, ONE_TRIP - 1, n - 100]),
                            ("its only newline in the tail's last byte", [n - 1])):
        text = text_with(n, newlines)
        assert want_last(text, 0, n) == newlines[-1] + 1
        assert last_newline(lib, text, 0, n) == newlines[-1] + 1, title
    text = text_with(n, [2, 83, n - 100, n - 6])
    assert last_newline(lib, text, 3, n - 7) == n - 99        # (lo and hi off the words' borders; the newlines at 2 and n - 6 do not count)
    assert last_newline(lib, text, 84, n - 100) == 0


def test_last_newline_at_offsets_above_4_gib(lib):
    """The text pointer is the buffer's address minus the offset of its first byte, as the decoder makes it: offsets of 2^32 and more
    on a buffer of a few words; the answer's high half is not zero, and the wave's maximum must compare all 64 bits."""
    four = G.FOUR_GIB

    def run(base, small, lo, hi):
        raw = small[:hi - base] + b"\n" * (((hi + 15) & ~15) - hi + S.PAD)
        buf = _dev(np.frombuffer(raw, np.uint8))
        d_last, _ = _inout(np.zeros(1, np.uint64))
        assert lib.spl_dev_launch_sam_last_newline(ctypes.c_void_p(buf.data_ptr() - base), ctypes.c_uint64(lo), ctypes.c_uint64(hi), _p(d_last), NULL) == 0
        torch.cuda.synchronize()
        got = int(_host(d_last, 8, np.uint64, "last")[0])
        want = small.rfind(b"\n", lo - base, hi - base)
        assert got == (base + want + 1 if want >= 0 else 0), (lo, hi, got)
        return got
    small = text_with(96, [2, 4, 9, 30, 44, 50, 70])
    assert run(four, small, four + 5, four + 50) == four + 45
    assert run(four, small, four + 5, four + 9) == 0
    assert run(four, small, four + 45, four + 96) == four + 71
    # a range across 2^32: a newline below it whose low half is large, one above whose low half is small
    base = four - 32
    assert run(base, text_with(96, [22, 35]), four - 20, four + 30) == four + 4
    assert run(base, text_with(96, [22]), four - 20, four + 30) == four - 9
    assert run(base, text_with(96, [31]), four - 20, four + 30) == four
    assert run(base, text_with(96, [32]), four - 20, four + 30) == four + 1


# ---- long_line ----------------------------------------------------------------------------------------------------------------------

MAX_LINE = 300


def first_long(lengths, max_line):
    for i, ln in enumerate(lengths):
        if ln > max_line:
            return i
    return NO_LINE


def run_long_line(lib, lengths, max_line=MAX_LINE, first=16):
    """Lines of these lengths, the first one ``first`` bytes behind the window's base -> *first_long."""
    lengths = np.asarray(lengths, np.int64)
    n = len(lengths)
    ends = first + np.cumsum(lengths)
    starts = np.concatenate(([first], ends[:-1])).astype(np.uint32) if n else np.zeros(0, np.uint32)
    d_start = _dev(starts) if n else _dev(np.zeros(1, np.uint32))
    d_long, _ = _inout(np.full(1, NO_LINE, np.uint32))
    assert lib.spl_dev_launch_sam_long_line(_p(d_start), ctypes.c_uint32(n), ctypes.c_uint32(int(ends[-1]) if n else first), ctypes.c_uint32(max_line), _p(d_long), NULL) == 0
    torch.cuda.synchronize()
    got = int(_host(d_long, 4, np.uint32, "first_long")[0])
    assert got == first_long(lengths.tolist(), max_line), (n, got)
    return got


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_long_line(lib, n):
    rng = np.random.default_rng(n)
    plain = rng.integers(1, MAX_LINE + 1, n)
    plain[rng.integers(0, n, 4)] = MAX_LINE                       # exactly max_line bytes: not long
    plain[0] = MAX_LINE
    assert run_long_line(lib, plain) == NO_LINE                   # ~0 is left as it was set
    for k in sorted({0, n // 2, n - 1, min(255, n - 1), min(256, n - 1)}):
        one = plain.copy()
        one[k] = MAX_LINE + 1
        assert run_long_line(lib, one) == k
    several = plain.copy()
    several[[n - 1, n // 2, n // 3, (2 * n) // 3]] = MAX_LINE + 1, MAX_LINE + 50, MAX_LINE + 1, 5 * MAX_LINE
    assert run_long_line(lib, several) == n // 3                  # the smallest index wins
    # the last line has no start behind it: end_off says where it ends
    last = plain.copy()
    last[-1] = MAX_LINE
    assert run_long_line(lib, last) == NO_LINE
    last[-1] = MAX_LINE + 1
    assert run_long_line(lib, last) == n - 1
    assert run_long_line(lib, plain, max_line=MAX_LINE - 1) == 0  # (line 0 has MAX_LINE bytes)
    assert run_long_line(lib, [0xFFFFFF00 - 16] * 1 + [0] * (n - 1), max_line=0xFFFFFF00 - 17) == 0   # (lengths that need all 32 bits)


def test_long_line_of_no_line_launches_nothing(lib):
    assert run_long_line(lib, []) == NO_LINE


# ---- order --------------------------------------------------------------------------------------------------------------------------

def want_unordered(tid, pos, first, n):
    return any(tid[r] < tid[r - 1] or (tid[r] == tid[r - 1] and pos[r] < pos[r - 1]) for r in range(max(first, 1), first + n))


def run_order(lib, tid, pos, first, n):
    tid, pos = np.asarray(tid, np.int32), np.asarray(pos, np.int32)
    assert first + n <= len(tid) == len(pos)
    d_tid, d_pos = _dev(tid), _dev(pos)
    d_counts, _ = _inout(np.zeros(1, COUNTS))
    assert lib.spl_dev_launch_sam_order(_p(d_tid), _p(d_pos), ctypes.c_uint64(first), ctypes.c_uint64(n), _p(d_counts), NULL) == 0
    torch.cuda.synchronize()
    got = _host(d_counts, COUNTS.itemsize, COUNTS, "counts")[0]
    assert [int(got[k]) for k in ("first_bad", "n_drop_flags", "n_drop_mapq", "overflow")] == [0, 0, 0, 0]
    assert int(got["unordered"]) in (0, 1)
    assert bool(got["unordered"]) == want_unordered(tid.tolist(), pos.tolist(), first, n), (first, n)
    return bool(got["unordered"])


@pytest.mark.parametrize("n", [1, 256, 257])
@pytest.mark.parametrize("first", [37, 300])
def test_order_of_a_window_behind_the_first(lib, first, n):
    assert first % 64 and first % 256
    total = first + n + 2                       # (two records behind the window: a descent there is the next window's)
    tid = np.repeat(np.arange(total // 50 + 1), 50)[:total].astype(np.int32)
    pos = (1000 + 3 * np.arange(total)).astype(np.int32)
    assert run_order(lib, tid, pos, first, n) is False

    def with_descent(at, what):
        t, p = tid.copy(), pos.copy()
        if what == "pos":                       # the same reference, POS goes down
            t[at - 1] = t[at]
            p[at] = p[at - 1] - 1
        elif what == "tid":                     # the reference id goes down, POS goes up
            t[:at] += 5
        tl, pl = t.tolist(), p.tolist()
        assert [r for r in range(1, total) if want_unordered(tl, pl, r, 1)] == [at]
        return t, p
    for what in ("pos", "tid"):
        assert run_order(lib, *with_descent(first, what), first, n) is True           # between first - 1 and first: this window's
        assert run_order(lib, *with_descent(first - 1, what), first, n) is False      # between first - 2 and first - 1: not
        assert run_order(lib, *with_descent(first + n - 1, what), first, n) is True   # the window's last record
        assert run_order(lib, *with_descent(first + n, what), first, n) is False      # the first one behind it
        assert run_order(lib, *with_descent(first + n // 2, what), first, n) is True
    # the reference id goes up and POS goes down: in order
    t, p = tid.copy(), pos.copy()
    t[first:] += 1
    p[first:] -= 900
    assert run_order(lib, t, p, first, n) is False
    # equal ids with equal POS: in order
    assert run_order(lib, np.full(total, 3), np.full(total, 77), first, n) is False
