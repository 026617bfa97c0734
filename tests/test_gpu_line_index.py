"""The line index the device's text sources share (spl_capi.cpp: LineIndex, through the hook ``spl_text_line_index``): ONE index over
windows of one text in an order that has its kept buffers made, outgrown, reused while larger than needed, filled to the last
line they have room for and outgrown by one line -- every window's line starts against ``samcases.line_starts``, the restatement
tests/test_gpu_sam_kernels.py holds the two kernels to.  Everything is exact."""
import numpy as np
import pytest

import samcases as S
from spliser_amd import native

pytestmark = pytest.mark.gpu


def line(n):
    return b"A" * (n - 1) + b"\n"


def build_text():
    """-> (text, {name: (lo, hi)})."""
    at, parts, win = 0, [], {}

    def add(b):
        nonlocal at
        parts.append(b)
        at += len(b)
        return at

    add(b"AAAA\n")
    win["ten_lines"] = (5, add(line(100) * 10))                     # one chunk, lo neither a multiple of 16 nor of a chunk
    add(b"A" * (2048 - at - 1) + b"\n")
    lo = at                                                         # three chunks and a byte; a line begins on the second chunk's first byte
    add(line(24) * 682 + line(16))
    assert at - lo == S.CHUNK
    win["three_chunks_and_a_byte"] = (lo, add(line(24) * 1365 + line(9)))
    assert at - lo == 3 * S.CHUNK + 1 and lo % 16 == 0
    add(b"A" * 6 + b"\n")
    lo = at                                                         # lines of two bytes: as many as the index has room for, and one more
    add(line(2) * 2306)
    win["room_exactly"], win["room_and_one"] = (lo, lo + 2 * 2305), (lo, lo + 2 * 2306)
    lo = at
    win["no_newline"] = (lo, add(b"A" * 77))                        # a last window: one line, the text ends without a newline
    return b"".join(parts), win


ORDER = ["ten_lines", "three_chunks_and_a_byte", "ten_lines", "room_exactly", "room_and_one", "no_newline"]


def test_one_index_over_windows_that_reuse_and_outgrow_its_buffers():
    native.build()
    text, win = build_text()
    want = {name: np.asarray(S.line_starts(text, lo, hi), np.int64) - (lo & ~15) for name, (lo, hi) in win.items()}
    assert [len(want[n]) for n in ORDER] == [10, 2049, 10, 2305, 2306, 1]
    assert 2049 + 2049 // 8 == 2305                                                       # (what the second window leaves room for)
    lo, hi = win["three_chunks_and_a_byte"]
    assert lo + S.CHUNK - (lo & ~15) in want["three_chunks_and_a_byte"] and text[hi - 1:hi] == b"\n"
    with native.Context(0) as ctx:
        got = native.text_line_index(ctx, text, [win[n] for n in ORDER])
    for name, (starts, room) in zip(ORDER, got):
        assert starts.dtype == np.uint32 and np.array_equal(starts.astype(np.int64), want[name]), name
    assert np.array_equal(got[0][0], got[2][0])                                           # the same answer from larger buffers
    assert [room for _, room in got] == [11, 2305, 2305, 2305, 2306 + 2306 // 8, 2306 + 2306 // 8]


def test_windows_outside_the_text_are_refused():
    native.build()
    with native.Context(0) as ctx:
        for w in ((0, 0), (3, 2), (0, 5), (-1, 2)):
            with pytest.raises(native.SpliserNativeError) as err:
                native.text_line_index(ctx, b"A\nA\n", [w])
            assert err.value.code == -1
