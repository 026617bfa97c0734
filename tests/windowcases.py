"""How a mapped text is cut into windows of whole lines (spliser_amd/csrc/spl_text_windows.h), restated from the header's words, and
the smallest texts at which a cut can go wrong.  ``motifcases.window_cuts`` stays the FASTA rule's restatement of its own; the test
holds the two against each other."""
import numpy as np

STOP, OWN = 0, 1     # what becomes of a line that fits no window: the plan stops in front of it (SAM text), a window of its own (FASTA)
W = 64               # the cases' window unless they say otherwise


def window_plan(text, begin, window, rule):
    """-> ([(lo, hi)], whether a line that fits no window stopped the plan).  A window is at most ``window`` bytes and ends behind
    the last newline among them; the last one ends with the text."""
    out, lo, n = [], begin, len(text)
    while lo < n:
        hi = min(n, lo + window)
        if hi < n:
            nl = text.rfind(b"\n", lo, hi)
            if nl < 0:
                if rule == STOP:
                    return out, True
                nl = text.find(b"\n", hi)
            hi = nl + 1 if nl >= 0 else n
        out.append((lo, hi))
        lo = hi
    return out, False


def line(n, end=b"\n"):
    """A line of n bytes, its end counted."""
    return b"A" * (n - len(end)) + end


def cases():
    """[(name, text, begin, window)], each for both rules."""
    short, over = line(20), line(W + 30)
    head = b"@HD\tVN:1.6\n@SQ\tSN:c\tLN:9\n"           # 25 bytes: a body that begins at no multiple of 16
    out = [
        ("empty_body", head, len(head), W),
        ("begin_inside", head + short * 9, len(head), W),
        ("begin_inside_a_window_exactly", head + line(W) + short, len(head), W),
        ("no_newline_shorter", b"A" * (W - 1), 0, W),
        ("no_newline_equal", b"A" * W, 0, W),
        ("no_newline_longer", b"A" * (W + 1), 0, W),
        ("newline_is_the_windows_last_byte", line(24) + line(40) + short * 3, 0, W),
        ("newline_is_the_first_byte_behind", line(11) + line(54) + short * 3, 0, W),
        ("line_of_a_window", line(W) + short * 2, 0, W),
        ("line_of_a_window_and_a_byte", line(W + 1) + short * 2, 0, W),
        ("line_of_a_window_later", short + line(W) + short, 0, W),
        ("line_of_a_window_and_a_byte_later", short + line(W + 1) + short, 0, W),
        ("long_first", over + short * 4, 0, W),
        ("long_in_the_middle", short * 4 + over + short * 4, 0, W),
        ("long_last_with_newline", short * 4 + over, 0, W),
        ("long_last_without_newline", short * 4 + over[:-1], 0, W),
        ("two_long_in_a_row", short * 2 + over + line(3 * W) + short * 2, 0, W),
        ("last_line_without_newline", short * 5 + b"AAAA", 0, W),
        ("last_line_without_newline_fills_a_window", short * 2 + b"A" * W, 0, W),
        ("crlf_cut_between", line(12, b"\r\n") + line(53, b"\r\n") + line(30, b"\r\n") * 3, 0, W),
        ("crlf_ends_a_window", line(24, b"\r\n") + line(40, b"\r\n") + line(30, b"\r\n") * 3, 0, W),
        ("only_newlines", b"\n" * (2 * W + 5), 3, W),
        ("window_larger_than_the_text", short * 7, 0, 4096),
        ("window_of_a_byte", b"A\n\nAA\n\n", 0, 1),
        ("header_only_then_long", head + over + short, len(head), W),
    ]
    text = out[7][1]
    assert text[W:W + 1] == b"\n" and out[6][1][W - 1:W] == b"\n"
    assert out[19][1][W - 1:W + 1] == b"\r\n" and out[20][1][W - 2:W] == b"\r\n"
    return out


def random_cases(n=400, seed=20):
    """Texts of at most 4 KiB over {A, newline, CR}, windows from 1..300, a begin inside every third text."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        size = int(rng.integers(0, 4097))
        p_nl = (0.3, 0.05, 0.01, 0.003)[k % 4]
        text = rng.choice(np.frombuffer(b"A\n\r", np.uint8), size=size, p=[1 - 1.5 * p_nl, p_nl, 0.5 * p_nl]).astype(np.uint8).tobytes()
        begin = int(rng.integers(0, size + 1)) if k % 3 == 0 else 0
        out.append(("random%d" % k, text, begin, int(rng.integers(1, 301))))
    return out


def check_plan(text, begin, window, rule, plan, long_line):
    """The properties of every plan, whoever made it."""
    end = begin
    for k, (lo, hi) in enumerate(plan):
        assert lo == end and hi > lo, (k, lo, hi)                  # the windows tile [begin, end) without gap or overlap
        end = hi
        if k + 1 < len(plan):
            assert text[hi - 1:hi] == b"\n", (k, lo, hi)           # every window but possibly the last ends behind a newline
        if rule == STOP:
            assert hi - lo <= window
        elif hi - lo > window:                                     # ... a window of its own: one line, and no window held it
            assert b"\n" not in text[lo:hi - 1] and (text[hi - 1:hi] == b"\n" or hi == len(text))
    if rule == OWN or not long_line:
        assert end == max(begin, len(text)) and not long_line      # under the FASTA rule the plan ends with the text
    else:
        assert end < len(text) and b"\n" not in text[end:end + window] and len(text) - end > window
