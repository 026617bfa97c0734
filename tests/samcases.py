"""Hand-built SAM texts and a plain Python statement of the strict rule (csrc/spl_sam_line.h), for test_samcases_host.py and the GPU
tests of the text decoder.  No tests in here.

``rule`` reads one line the way the header says a line is read -- ``bytes.split``, regular expressions and ``int`` -- and shares
nothing with the C function but the header's words; ``reference`` applies it to a whole case: the line starts, what every line
gives, the arrays in file order and per reference in the order the decoders hand them out, the counters, and where the file is
declined.  ``twin`` writes the BAM of the same records (reference ids, mates and XS tags included), for the claim that the text
decoder counts what the BAM decoder counts.

The kernels' geometry, read from csrc/spl_sam.h: a wave per chunk of 16 KiB, lanes of 16 bytes, chunk k beginning at (lo & ~15) +
k * 16 KiB.  Every case's header is padded so that the alignment lines begin at a multiple of 16 KiB + ``lead`` bytes: the shapes
below say where a newline falls in a lane's word and in a chunk."""
import os
import re
import struct

import numpy as np

import flagstatcases as fs
import scancases as sc
from spliser_amd import samio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spliser_amd", "csrc")


def _defines(path, prefix):
    with open(os.path.join(CSRC, path)) as fh:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+%s(\w+)\s+(\d+)u" % prefix, fh.read())}


R = _defines("spl_sam_line.h", "SPL_SAM_")          # reason codes: R["BAD_FLAG"], ...
_GEOMETRY = _defines("spl_sam.h", "SPL_SAM_")
CHUNK, PAD, SCAN_LANES = _GEOMETRY["CHUNK"], _GEOMETRY["PAD"], _GEOMETRY["SCAN_LANES"]
assert CHUNK == 16384 and PAD == 16, "the cases below are laid out for chunks of 16 KiB and lanes of 16 bytes"
with open(os.path.join(CSRC, "spl_sam_line.h")) as _fh:
    REASON_TEXT = re.search(r"text\[SPL_SAM_N_REASONS\] = \{(.*?)\};", _fh.read(), re.S).group(1)
REASON_TEXT = re.findall(r'"([^"]*)"', REASON_TEXT)
assert len(REASON_TEXT) == R["N_REASONS"]

KEPT, DROP_FLAGS, DROP_MAPQ = 0, 1, 2
_OPS = b"MIDNSHP=X"


# ---- the rule, said once more ----------------------------------------------------------------------------------------------
def _number(col, digits, limit):
    if not re.fullmatch(rb"[0-9]{1,%d}" % digits, col):
        return None
    v = int(col)
    return v if v <= limit else None


def rule(line, tid_of, filt=(0, 0, 0)):
    """One line (bytes, without its newline) -> (reason, None) or (0, dict of what the rule reads off it)."""
    if line == b"":
        return R["EMPTY"], None
    if line[:1] == b"@":
        return R["LATE_HEADER"], None
    if b"\r" in line:
        return R["CR"], None
    cols = line.split(b"\t")
    if len(cols) < 11:
        return R["COLUMNS"], None
    flag = _number(cols[1], 5, 65535)
    if flag is None:
        return R["BAD_FLAG"], None
    tid = -1 if cols[2] == b"*" else tid_of.get(cols[2])
    if tid is None:
        return R["BAD_RNAME"], None
    pos = _number(cols[3], 10, 2 ** 31 - 1)
    if pos is None:
        return R["BAD_POS"], None
    mapq = _number(cols[4], 3, 255)
    if mapq is None:
        return R["BAD_MAPQ"], None
    if cols[5] == b"*":
        ops = []
    else:
        if not re.fullmatch(rb"(?:[0-9]{1,9}[MIDNSHP=X])+", cols[5]):
            return R["BAD_CIGAR"], None
        pairs = re.findall(rb"([0-9]+)([MIDNSHP=X])", cols[5])
        if any(int(n) >= 1 << 28 for n, _ in pairs):
            return R["BAD_CIGAR"], None
        ops = [int(n) << 4 | _OPS.index(c) for n, c in pairs]
    next_tid = tid if cols[6] == b"=" else -1 if cols[6] == b"*" else tid_of.get(cols[6])
    if next_tid is None:
        return R["BAD_RNEXT"], None
    if tid >= 0 and pos == 0:
        return R["POS_ZERO"], None
    q, f, F = filt
    verdict = DROP_FLAGS if (flag & F) or (flag & f) != f else (KEPT if mapq >= q else DROP_MAPQ)
    placed = tid >= 0
    ref_len = sum(o >> 4 for o in ops if (o & 15) in (0, 2, 3, 7, 8))
    xs = samio.sam_aux_strand(cols[5].decode("ascii"), [c.decode("latin-1") for c in cols[11:]]) if placed else 0
    return 0, dict(flag=flag, tid=tid, pos=pos, mapq=mapq, ops=ops if placed else [], next_tid=next_tid, verdict=verdict, placed=placed, xs=xs,
                   end=pos + max(ref_len, 1) - 1)


def line_starts(text, lo, hi):
    """Where lines begin in text[lo:hi): at lo, and behind every newline that is not the last byte."""
    if hi <= lo:
        return []
    at = np.flatnonzero(np.frombuffer(text, np.uint8)[lo:hi] == 10) + lo + 1
    return [lo] + [int(p) for p in at if p < hi]


class Reference(object):
    """What the decoders must leave for a case (``reference``)."""


def reference(case):
    if case.name in _REFERENCE:
        return _REFERENCE[case.name]
    text, lo, hi = case.text(), case.begin, len(case.text())
    tid_of = {n.encode("ascii"): k for k, n in enumerate(case.ref_names)}
    ref = Reference()
    ref.starts = line_starts(text, lo, hi)
    ends = [s - 1 for s in ref.starts[1:]] + [hi - 1 if hi > lo and text[hi - 1:hi] == b"\n" else hi]
    ref.last_end = ends[-1] if ends else hi
    ref.lines, ref.decline = [], None
    for k, (s, e) in enumerate(zip(ref.starts, ends)):
        reason, got = rule(text[s:e], tid_of, case.filt)
        ref.lines.append((reason, got))
        if reason and ref.decline is None:
            ref.decline = (case.header_lines + k + 1, reason)
    good = [g for reason, g in ref.lines if not reason]
    ref.n_records = len(good)
    ref.dropped = [sum(1 for g in good if g["placed"] and g["verdict"] == v) for v in (DROP_FLAGS, DROP_MAPQ)]
    counted = [g for g in good if g["verdict"] == KEPT]
    ref.flagstat = fs.restate(*[[g[k] for g in counted] for k in ("flag", "tid", "next_tid", "mapq")]) if counted else np.zeros((16, 2), np.int64)
    kept = [g for g in good if g["placed"] and g["verdict"] == KEPT]
    ref.kept_mask = [int(not reason and g["placed"] and g["verdict"] == KEPT) for reason, g in ref.lines]
    ref.tid = np.array([g["tid"] for g in kept], np.int32)
    ref.pos = np.array([g["pos"] for g in kept], np.int32)
    ref.flag = np.array([g["flag"] for g in kept], np.uint16)
    ref.xs = np.array([g["xs"] for g in kept], np.uint8)
    ref.cig_off = np.concatenate(([0], np.cumsum([len(g["ops"]) for g in kept]))).astype(np.uint32)
    ref.cigar = np.array([o for g in kept for o in g["ops"]], np.uint32)
    key = ref.tid.astype(np.int64) << 32 | ref.pos.astype(np.int64)
    ref.unordered = bool(np.any(key[1:] < key[:-1]))
    ref.max_end = [max([g["end"] for g in kept if g["tid"] == t], default=0) for t in range(len(case.ref_names))]
    # per reference in file order (read_sam's), and as the decoders hand the reads out: file order, or -- reference ids or POS ever
    # going down -- stable by POS
    ref.per_ref_file, ref.per_ref = {}, {}
    for t, name in enumerate(case.ref_names):
        for into, by_pos in ((ref.per_ref_file, False), (ref.per_ref, ref.unordered)):
            idx = np.flatnonzero(ref.tid == t)
            if by_pos:
                idx = idx[np.argsort(ref.pos[idx], kind="stable")]
            ops = [ref.cigar[ref.cig_off[i]:ref.cig_off[i + 1]] for i in idx]
            into[name] = dict(pos=ref.pos[idx], flag=ref.flag[idx], xs=ref.xs[idx], cig_off=np.concatenate(([0], np.cumsum([len(o) for o in ops]))).astype(np.uint32),
                              cigar=np.concatenate(ops).astype(np.uint32) if ops else np.zeros(0, np.uint32), max_end=ref.max_end[t])
    _REFERENCE[case.name] = ref
    return ref


_REFERENCE = {}


# ---- builders --------------------------------------------------------------------------------------------------------------
def ln(q=b"r", flag=0, rname=b"chr1", pos=100, mapq=60, cigar=b"50M", rnext=b"*", pnext=0, tlen=0, seq=b"*", qual=b"*", tags=()):
    """One alignment line's bytes, without the newline; every column as given (numbers as ints or as bytes)."""
    cols = [q, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual] + list(tags)
    return b"\t".join(c if isinstance(c, bytes) else str(c).encode("ascii") for c in cols)


def fit(n, **kw):
    """A line of exactly n bytes, its newline counted: SEQ takes up the slack."""
    bare = len(ln(seq=b"", **kw)) + 1
    assert n >= bare + 1, "no line that short"
    return ln(seq=b"A" * (n - bare), **kw)


class Case(object):
    """A SAM file: header (@HD, @SQ per name, an @CO line that pads it so that the lines begin ``lead`` bytes behind a multiple of
    16 KiB), the lines, each with its newline but -- ``final_nl=False`` -- the last.  ``window``: SPL_SAM_WINDOW_BYTES for the
    decoders (None: the default).  ``twin``: the BAM decoder takes the same records (``write_twin``)."""

    def __init__(self, name, lines, ref_names=("chr1", "chr2"), final_nl=True, filt=(0, 0, 0), window=None, lead=0, twin=True, what="", ref_len=2 ** 31 - 1):
        self.ref_len = ref_len
        self.name, self.lines, self.ref_names, self.final_nl, self.filt, self.window, self.twin, self.what = name, list(lines), list(ref_names), final_nl, tuple(filt), window, twin, what
        head = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n.encode("ascii"), ref_len) for n in self.ref_names)
        room = -(len(head) + 5 - lead) % CHUNK          # "@CO\t" and its newline are five bytes
        self.header = head + b"@CO\t" + b"x" * room + b"\n"
        self.begin = len(self.header)
        assert self.begin % CHUNK == lead
        self.header_lines = self.header.count(b"\n")
        self._text = None

    def text(self):
        if self._text is None:
            body = b"\n".join(self.lines) + (b"\n" if self.lines and self.final_nl else b"")
            self._text = self.header + body
        return self._text

    def write(self, path):
        with open(path, "wb") as fh:
            fh.write(self.text())
        return str(path)


_TAG = re.compile(rb"([A-Za-z][A-Za-z0-9]):([AiZ]):(.*)", re.S)


def write_twin(case, path, shuffle=None):
    """The BAM of the case's records (every line must be one the rule takes): same reference ids, mates, MAPQs and -- as aux fields
    -- the lines' tags of type A, i and Z.  ``shuffle``: a permutation of the lines."""
    tid_of = {n.encode("ascii"): k for k, n in enumerate(case.ref_names)}
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, case.ref_len) for n in case.ref_names)
    stream = [b"BAM\x01", struct.pack("<i", len(text)), text.encode("ascii"), struct.pack("<i", len(case.ref_names))]
    for n in case.ref_names:
        stream += [struct.pack("<i", len(n) + 1), n.encode("ascii") + b"\x00", struct.pack("<i", case.ref_len)]
    order = range(len(case.lines)) if shuffle is None else shuffle
    for k in order:
        line = case.lines[k]
        reason, g = rule(line, tid_of)
        assert reason == 0, (case.name, k, reason)
        cols = line.split(b"\t")
        aux = b""
        for field in cols[11:]:
            m = _TAG.fullmatch(field)
            assert m, field
            tag, ty, val = m.groups()
            aux += tag + (b"A" + val[:1] if ty == b"A" else b"i" + struct.pack("<i", int(val)) if ty == b"i" else b"Z" + val + b"\x00")
        ops = g["ops"] if g["placed"] else []
        assert len(ops) <= 65535, "a CIGAR for a CG tag: not a twin case"
        stream.append(sc.record(tid=g["tid"], pos=g["pos"] - 1, name=cols[0][:200] + b"\x00", mapq=g["mapq"], flag=g["flag"], cigar=ops, next_tid=g["next_tid"],
                                next_pos=int(cols[7]) - 1, aux=aux))
    stream = b"".join(stream)
    with open(path, "wb") as fh:
        for at in range(0, len(stream), samio._BGZF_BLOCK):
            fh.write(samio._bgzf_block(stream[at:at + samio._BGZF_BLOCK], 1))
        fh.write(samio._BGZF_EOF)
    return str(path)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def _spliced(k, rname=b"chr1", **kw):
    return ln(q=b"s%d" % k, rname=rname, pos=1000 + 7 * k, cigar=b"20M%dN30M" % (100 + k), **kw)


def shape_cases():
    """Where newlines fall: the smallest texts at which the line-start kernels, the windows and the arrays' growth can go wrong."""
    rng = np.random.default_rng(7)
    out = []
    out.append(Case("nl_first_of_word", [fit(33, pos=5), fit(48, pos=6), ln(pos=7)], what="a newline as the first byte of a lane's word, twice"))
    out.append(Case("nl_last_of_word", [fit(32, pos=5), fit(48, pos=6), ln(pos=7)], what="a newline as the last byte of a lane's word"))
    out.append(Case("nl_last_of_chunk", [fit(CHUNK // 2, pos=5), fit(CHUNK // 2, pos=6), ln(pos=7), ln(pos=8)], what="a line beginning at byte 0 of the second chunk"))
    out.append(Case("long_lines", [ln(pos=5), fit(CHUNK + 3000, pos=6), ln(pos=7), fit(3 * CHUNK + 5000, pos=8), ln(pos=9)], what="chunks without a line start"))
    out.append(Case("unaligned_begin", [fit(33, pos=5), fit(CHUNK - 40, pos=6), ln(pos=7)], lead=7, what="the lines begin seven bytes into a lane's word"))
    out.append(Case("ends_at_chunk", [fit(CHUNK, pos=5), fit(CHUNK - 100, pos=6), fit(100, pos=7)], what="the text ends exactly at a chunk boundary"))
    out.append(Case("no_final_newline", [ln(pos=5), _spliced(1, tags=[b"NH:i:1", b"XS:A:+"])], final_nl=False, what="the last line without its newline, XS:A:+ its last bytes"))
    out.append(Case("single_line", [ln(pos=5)]))
    out.append(Case("single_line_bare", [ln(pos=5)], final_nl=False))
    out.append(Case("header_only", []))
    # windows: the host cuts them behind a line's end, so a line is never in two -- and a line longer than a window is declined
    body = [fit(300 + int(rng.integers(0, 40)), q=b"w%d" % k, pos=10 + k, flag=int(rng.choice([0, 16, 99, 147]))) for k in range(60)]
    out.append(Case("windows_4k", body, window=4096, what="five windows; lines that would straddle them"))
    out.append(Case("line_fills_window", [ln(pos=5), fit(4096, pos=6), ln(pos=7)], window=4096, what="a line of exactly a window"))
    return out


def large_case():
    """About 3 000 lines of ~300 bytes on three references, then as many short ones: some sixty chunks, four windows of 256 KiB, and
    output arrays that must grow (the first window's density says 850 reads for its bytes, the second half has five times that)."""
    rng = np.random.default_rng(11)
    names = ("chr1", "chr10", "chr1_random")
    lines, pos = [], 1
    for k in range(3000):
        pos += int(rng.integers(0, 30))
        r = names[min(k // 1000, 2)].encode("ascii")
        flag = int(rng.choice([0, 16, 99, 147, 83, 163, 256, 1024 + 99, 512 + 147, 4 + 73, 2048 + 16]))
        cigar = b"%dM%dN%dM" % (20 + k % 7, 100 + k % 900, 30) if k % 3 == 0 else b"%dM2I%dM" % (25, 23) if k % 3 == 1 else b"50M"
        tags = [b"NH:i:%d" % (1 + k % 3)] + ([b"XS:A:%s" % (b"+" if k % 2 else b"-")] if k % 3 == 0 else [])
        rnext = (b"=", b"*", b"chr10")[k % 3]
        lines.append(fit(290 + int(rng.integers(0, 30)), q=b"a%d" % k, flag=flag, rname=r, pos=pos, mapq=int(rng.choice([0, 1, 3, 20, 60, 255])), cigar=cigar, rnext=rnext,
                         pnext=pos + 200, qual=b"*", tags=tags))
        if k % 1000 == 999:
            pos = 1
    for k in range(3000):
        lines.append(ln(q=b"b%d" % k, rname=b"chr1_random", pos=40000 + k, cigar=b"10M", flag=16 * (k % 2)))
    for k in range(5):
        lines.append(ln(q=b"u%d" % k, flag=4 + 512 * (k % 2), rname=b"*", pos=0, mapq=0, cigar=b"*"))
    return Case("large", lines, ref_names=names, window=256 << 10, ref_len=10 ** 6, what="four windows, arrays regrown")


def field_cases():
    """The numbers, CIGARs, names and tags at their limits -- all lines the rule takes."""
    out = []
    out.append(Case("numbers", [ln(flag=0, pos=1, mapq=0), ln(flag=65535, pos=2 ** 31 - 1, mapq=254, cigar=b"*"), ln(flag=99, pos=7, mapq=255, rnext=b"="),
                                ln(flag=4, rname=b"*", pos=500, mapq=3, cigar=b"*"), ln(flag=77, rname=b"*", pos=0, mapq=0, cigar=b"*", rnext=b"chr2")],
                    what="FLAG 0 and 65535, POS 1 and 2^31 - 1, MAPQ 0 / 254 / 255, '*' with a POS"))
    for q in (254, 255):
        out.append(Case("minmapq_%d" % q, out[0].lines, filt=(q, 0, 0), what="MAPQ 254 and 255 against --minMapQ %d" % q))
    out.append(Case("flag_filter", out[0].lines + [ln(flag=1024, pos=9, mapq=0)], filt=(1, 0, 1024), what="flags are tested first"))
    every = b"5M1I2D100N3S4H1P6=7X"
    out.append(Case("cigars", [ln(cigar=b"*", pos=5), ln(cigar=b"1M", pos=6), ln(cigar=b"%dM" % (2 ** 28 - 1), pos=7), ln(cigar=every, pos=8),
                               ln(cigar=b"000000005M", pos=9)], what="'*', one op, an op of 2^28 - 1, all nine letters, nine digits"))
    out.append(Case("many_ops", [ln(pos=5), ln(pos=6, cigar=b"1M1N" * 35000, tags=[b"XS:A:-"]), ln(pos=7)], twin=False, what="a read of 70 000 ops"))
    names = ["chr1", "chr10", "chr1_random", "c", "L" * 200] + ["scaffold_%d" % k for k in range(1000)]
    lines = [ln(rname=n.encode("ascii"), pos=5 + k, rnext=(b"=", b"*", names[(k * 7) % len(names)].encode("ascii"))[k % 3], flag=1 + 64) for k, n in enumerate(names)]
    out.append(Case("names", lines, ref_names=names, what="chr1 / chr10 / chr1_random, one byte, 200 bytes, a thousand names; RNEXT '=', '*', another"))
    sp = dict(cigar=b"20M100N30M")
    out.append(Case("xs", [ln(pos=5, tags=[b"XS:A:+", b"NH:i:1"], **sp), ln(pos=6, tags=[b"XS:i:5", b"XS:A:-"], **sp), ln(pos=7, tags=[b"XS:A:?"], **sp),
                           ln(pos=8, tags=[b"XS:A:+"]), ln(pos=9, tags=[b"CO:Z:XS:A:+"], **sp), ln(pos=10, tags=[b"NH:i:1", b"XS:A:+", b"XS:A:-"], **sp),
                           ln(pos=12, rname=b"chr2", tags=[b"NH:i:2", b"XS:A:-"], **sp)],
                    what="XS:A first and last, XS:i in front, '?', on an unspliced read, inside a CO:Z string"))
    out.append(Case("xs_text_only", [ln(pos=11, tags=[b"XS:A:+-"], **sp), ln(pos=12, tags=[b"XS:A:"], **sp), ln(pos=13, tags=[b"xs:A:+", b"XS:A:-"], **sp)], twin=False,
                    what="values no BAM field of type A can hold: two bytes, none"))
    return out


def decline_cases():
    """One file per reason the rule declines: two good lines, the bad one, a good one -> (case, line number, reason)."""
    ok = [ln(pos=5), ln(pos=6)]
    bad = [("ten_columns", b"\t".join(ln().split(b"\t")[:10]), "COLUMNS"), ("signed_flag", ln(flag=b"+5"), "BAD_FLAG"), ("blank_flag", ln(flag=b" 5"), "BAD_FLAG"),
           ("flag_65536", ln(flag=65536), "BAD_FLAG"), ("empty_flag", ln(flag=b""), "BAD_FLAG"), ("pos_2_31", ln(pos=2 ** 31), "BAD_POS"), ("signed_pos", ln(pos=b"-1"), "BAD_POS"),
           ("mapq_256", ln(mapq=256), "BAD_MAPQ"), ("unknown_rname", ln(rname=b"chr3"), "BAD_RNAME"), ("prefix_rname", ln(rname=b"chr"), "BAD_RNAME"),
           ("unknown_rnext", ln(rnext=b"chrX"), "BAD_RNEXT"), ("pos_zero", ln(pos=0), "POS_ZERO"), ("cigar_B", ln(cigar=b"5B"), "BAD_CIGAR"), ("cigar_M5", ln(cigar=b"M5"), "BAD_CIGAR"),
           ("cigar_5", ln(cigar=b"5"), "BAD_CIGAR"), ("cigar_5M3", ln(cigar=b"5M3"), "BAD_CIGAR"), ("cigar_2_28", ln(cigar=b"%dM" % 2 ** 28), "BAD_CIGAR"),
           ("cigar_ten_digits", ln(cigar=b"0000000005M"), "BAD_CIGAR"), ("cigar_empty", ln(cigar=b""), "BAD_CIGAR"), ("empty_line", b"", "EMPTY"),
           ("late_header", b"@CO\tlate", "LATE_HEADER"), ("carriage_return", ln(cigar=b"20M100N30M", tags=[b"XS:A:+\r"]), "CR")]
    out = []
    for name, line, reason in bad:
        case = Case("decline_" + name, ok + [line, ln(pos=9)], twin=False)
        out.append((case, case.header_lines + 3, R[reason]))
    case = Case("decline_long_line", [ln(pos=5), fit(4097, pos=6), ln(pos=7)], window=4096, twin=False)     # (the driver's: the rule itself takes every line)
    out.append((case, case.header_lines + 2, R["LONG_LINE"]))
    case = Case("decline_bad_before_long", [ln(pos=5), ln(flag=b"x"), fit(4097, pos=6), ln(pos=7)], window=4096, twin=False)     # (the first line not taken is the one reported)
    out.append((case, case.header_lines + 2, R["BAD_FLAG"]))
    case = Case("decline_last_line", ok + [ln(flag=b"x")], final_nl=False, twin=False)
    out.append((case, case.header_lines + 3, R["BAD_FLAG"]))
    return out


def shuffled(case, seed=3):
    """The case's lines in a random order -> (the case, the permutation)."""
    perm = [int(k) for k in np.random.default_rng(seed).permutation(len(case.lines))]
    return Case(case.name + "_shuffled", [case.lines[k] for k in perm], ref_names=case.ref_names, final_nl=case.final_nl, filt=case.filt, window=case.window, twin=case.twin, ref_len=case.ref_len), perm


def accepted_cases():
    large = large_case()
    return shape_cases() + field_cases() + [large, shuffled(large)[0]]


def all_lines():
    """Every line of every case, each once (the sanitizer program's input): the 70 000-op read and the lines of several chunks too."""
    seen, out = set(), []
    for case in accepted_cases() + [c for c, _, _ in decline_cases()]:
        for line in case.lines:
            if (tuple(case.ref_names), case.filt, line) not in seen:
                seen.add((tuple(case.ref_names), case.filt, line))
                out.append((case, line))
    return out
