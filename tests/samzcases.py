"""Compressed SAM text for the tests of the compressed-text decoders (test_samz_host.py, test_gpu_samz.py): a text written as BGZF
with chosen payload cut points and level, or as gzip with chosen member cuts.  No tests in here.

``snapshot``: everything a decode leaves, for a comparison of two decodes of the same text.  ``bgzf(text, cuts)``: block k holds text[cuts[k - 1]:cuts[k]] (a cut point given twice is an empty block, ISIZE 0), then the EOF
marker.  ``gz(text, cuts)``: one gzip member per piece.  ``FORMS``: the four ways every case of samcases.py is written -- BGZF at
level 1 and stored (level 0), gzip in one member and in two cut in the middle of a line."""
import gzip
import io

from spliser_amd import samio

BLOCK = 1021        # payload bytes of the cases' blocks: a prime, so that block edges fall anywhere in lines, lanes' words and chunks


def bgzf(text, cuts=None, level=1, block=BLOCK, eof=True):
    if cuts is None:
        cuts = list(range(block, len(text), block))
    edges = [0] + list(cuts) + [len(text)]
    assert all(a <= b for a, b in zip(edges, edges[1:])), "cut points go up"
    out = [samio._bgzf_block(text[a:b], level) for a, b in zip(edges, edges[1:])]
    return b"".join(out) + (samio._BGZF_EOF if eof else b"")


def gz(text, cuts=(), level=6):
    edges = [0] + list(cuts) + [len(text)]
    out = []
    for a, b in zip(edges, edges[1:]):
        buf = io.BytesIO()
        with gzip.GzipFile(fileobj=buf, mode="wb", compresslevel=level, mtime=0) as fh:
            fh.write(text[a:b])
        out.append(buf.getvalue())
    return b"".join(out)


def mid_line_cut(case):
    """An offset inside a line of the case's text (inside the header where there are no lines): not behind a newline, not at one."""
    text = case.text()
    at = case.begin + (len(text) - case.begin) // 2
    while at < len(text) - 1 and (text[at - 1:at] == b"\n" or text[at:at + 1] == b"\n"):
        at += 1
    if at >= len(text) - 1:
        at = case.begin // 2
    return at


FORMS = {
    "bgzf1": lambda case: bgzf(case.text(), level=1),
    "bgzf0": lambda case: bgzf(case.text(), level=0),
    "gzip1": lambda case: gz(case.text()),
    "gzip2": lambda case: gz(case.text(), [mid_line_cut(case)]),
}
KIND = {"bgzf1": "BGZF", "bgzf0": "BGZF", "gzip1": "gzip", "gzip2": "gzip"}


def write(path, data):
    with open(str(path), "wb") as fh:
        fh.write(data)
    return str(path)


def snapshot(sam, case):
    """Everything a decode leaves, for a comparison of two decodes of the same text."""
    out = dict(declined=sam.declined())
    if out["declined"]:
        return out
    out.update(n=sam.n_records, dropped=list(sam.filter_counts()), flagstat=sam.flagstat().tolist(), sorted=sam.any_order_sorted(), names=list(sam.ref_names))
    for name in case.ref_names[:40] + case.ref_names[-3:]:
        r = sam.reads(name)
        out[name] = (sam.wait_ref(name), None if r is None else [None if getattr(r, k) is None else getattr(r, k).tolist() for k in ("pos", "flag", "cig_off", "cigar", "xs")])
    return out
