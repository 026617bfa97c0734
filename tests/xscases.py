"""Shared by the tests of ``--strandFromXS``: the yardstick for a strand byte (a walk over a BAM record's aux area written from
the SAM specification, section 4.2.4), aux areas to hold the decoders to it, read sets with mixed tags, and the yardstick for a
mode-3 junction table composed from ``oracle.junction_table`` (the reads split by their strand byte, the table of every group
with ``stranded=0``, the ``?`` of the tagged groups relabelled, merged and sorted).  Nothing here touches the GPU."""
import struct

import numpy as np

from oracle import oracle
from spliser_amd import samio

_FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
_ELEM = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def py_walk(aux):
    """-> ord('+'), ord('-') or 0: the value of the first XS:A field of the area, if it can be walked to and is + or -."""
    p, end = 0, len(aux)
    while end - p >= 3:
        tag, ty = aux[p:p + 2], chr(aux[p + 2])
        p += 3
        if ty in _FIXED:
            size = _FIXED[ty]
        elif ty in "ZH":
            nul = aux.find(b"\x00", p)
            if nul < 0:
                return 0
            size = nul - p + 1
        elif ty == "B":
            if end - p < 5 or chr(aux[p]) not in _ELEM:
                return 0
            size = 5 + struct.unpack_from("<I", aux, p + 1)[0] * _ELEM[chr(aux[p])]
        else:
            return 0
        if end - p < size:
            return 0
        if tag == b"XS" and ty == "A":
            return aux[p] if aux[p:p + 1] in (b"+", b"-") else 0
        p += size
    return 0


def field(tag, ty, value=None, sub=None, rng=None):
    """One well-formed aux field as bytes."""
    head = tag + ty.encode()
    if ty == "A":
        return head + (value if value is not None else b"x")
    if ty in _FIXED:
        return head + (value if value is not None else bytes(rng.integers(0, 256, _FIXED[ty], dtype=np.uint8)) if rng is not None else b"\x01" * _FIXED[ty])
    if ty in "ZH":
        return head + value + b"\x00"
    n = len(value) // _ELEM[sub]
    return head + sub.encode() + struct.pack("<I", n) + value


def star_area(xs=b"+"):
    """The five tags STAR writes with --outSAMstrandField intronMotif: NH HI AS nM XS."""
    return b"NHC\x01" + b"HIC\x01" + b"ASC\x62" + b"nMC\x00" + (b"XSA" + xs if xs is not None else b"")


def random_area(rng):
    """A well-formed area of 0..7 fields: any type, XS of any type among them, 'XSA+' bytes hidden in strings and arrays."""
    out = b""
    for _ in range(int(rng.integers(0, 8))):
        kind = int(rng.integers(0, 12))
        tag = bytes(rng.choice(list(b"XSNHASnMab"), 2).astype(np.uint8)) if kind % 3 else b"XS"
        if kind < 3:
            out += field(tag, "A", bytes([int(rng.choice(list(b"+-.?*")))]))
        elif kind < 6:
            out += field(tag, str(rng.choice(list("cCsSiIf"))), rng=rng)
        elif kind < 8:
            out += field(tag, str(rng.choice(list("ZH"))), bytes(rng.choice(list(b"XSA+-ab12"), int(rng.integers(0, 9))).astype(np.uint8)))
        else:
            sub = str(rng.choice(list("cCsSiIf")))
            n = int(rng.integers(0, 5))
            body = bytes(rng.choice(list(b"XSA+-\x01"), n * _ELEM[sub]).astype(np.uint8))
            out += field(tag, "B", body, sub=sub)
    return out


# what the aligners write, and what must not be taken for it: (aux bytes, the strand byte of a spliced read that carries them)
TAG_KINDS = [
    (star_area(b"+"), ord("+")),
    (star_area(b"-"), ord("-")),
    (star_area(None), 0),                                              # no XS at all
    (b"NMC\x00" + b"XSi" + struct.pack("<i", 37), 0),                    # BWA's XS:i, the suboptimal score
    (b"XSi" + struct.pack("<i", 43) + b"XSA-", ord("-")),              # ... stepped over on the way to an XS:A
    (star_area(b"."), 0),
    (b"COZXSA+\x00" + b"ZBBC" + struct.pack("<I", 4) + b"XSA+", 0),  # the bytes inside a string and an array
    (b"XSA+" + b"XSA-", ord("+")),                                     # the first wins
    (b"", 0),
]


def make_reads(rng, n, span=150000, n_junctions=30, long_cigar_every=0):
    """A coordinate-sorted ReadSet: four reads in ten spliced over a small set of junctions (so that every junction has several
    reads and the strands can mix), one or two N ops, soft clips, a few unmapped-but-placed."""
    lefts = np.sort(rng.integers(2000, span, n_junctions))
    lens = rng.integers(60, 3000, n_junctions)
    recs = []
    for i in range(n):
        if rng.random() < 0.6:
            recs.append((int(rng.integers(1, span)), "%dM" % int(rng.integers(30, 101))))
            continue
        j = int(rng.integers(0, n_junctions))
        a, b = int(rng.integers(1, 60)), int(rng.integers(1, 60))
        cigar = "%dM%dN%dM" % (a, int(lens[j]), b)
        if rng.random() < 0.2:
            cigar = "%dS" % int(rng.integers(1, 9)) + cigar + "%dN%dM" % (int(rng.integers(70, 900)), int(rng.integers(1, 40)))
        if long_cigar_every and i % long_cigar_every == 0:
            cigar = "".join("1M1I" for _ in range(40)) + cigar
            a += 40
        recs.append((int(lefts[j]) - a + 1, cigar))
    recs.sort(key=lambda r: r[0])
    flags = rng.choice([0, 16, 99, 147, 83, 163, 256, 4], n, p=[.3, .3, .08, .08, .08, .08, .06, .02])
    return samio.ReadSet.from_records([(int(f), p, c) for f, (p, c) in zip(flags, recs)])


def has_n(rs):
    code = rs.cigar & 15
    csum = np.concatenate(([0], np.cumsum(code == 3)))
    return (csum[rs.cig_off[1:].astype(np.int64)] - csum[rs.cig_off[:-1].astype(np.int64)]) > 0


def make_tags(rng, rs):
    """-> (aux bytes per read, the strand byte the decode must leave per read): every kind on spliced and unspliced reads alike."""
    kinds = rng.choice(len(TAG_KINDS), rs.n, p=[.3, .25, .15, .08, .05, .05, .04, .04, .04])
    tags = [TAG_KINDS[k][0] for k in kinds]
    want = np.where(has_n(rs), np.array([TAG_KINDS[k][1] for k in kinds]), 0).astype(np.uint8)
    return tags, want


def expected_xs(rs, tags):
    return np.where(has_n(rs), np.array([py_walk(t) for t in tags]), 0).astype(np.uint8)


def subset(rs, mask):
    idx = np.flatnonzero(mask)
    off = [0]
    ops = []
    for i in idx:
        ops.extend(rs.cigar[rs.cig_off[i]:rs.cig_off[i + 1]].tolist())
        off.append(len(ops))
    return samio.ReadSet(rs.pos[idx], rs.flag[idx], np.asarray(off, np.int64), np.asarray(ops, np.int64))


def yardstick(rs, xs, knobs=(0, 0, 0)):
    """The mode-3 table of (reads, strand bytes): rows (left, right, strand byte, count, anchor_left, anchor_right), sorted."""
    rows = []
    for byte, label in ((ord("+"), ord("+")), (ord("-"), ord("-")), (0, ord("?"))):
        sub = subset(rs, np.asarray(xs) == byte)
        for (l, r, s, n, al, ar) in oracle.junction_table(sub.pos, sub.flag, sub.cig_off, sub.cigar, 0, *knobs):
            assert s == ord("?")
            rows.append((l, r, label, n, al, ar))
    return sorted(rows)


def rows_of(table):
    return list(zip(*[np.asarray(table[k]).tolist() for k in ("left", "right", "strand", "count", "anchor_left", "anchor_right")]))


def table_of(rows):
    cols = list(zip(*rows)) if rows else [[]] * 6
    dts = (np.int32, np.int32, np.uint8, np.uint32, np.uint32, np.uint32)
    return {k: np.asarray(c, dt) for k, c, dt in zip(("left", "right", "strand", "count", "anchor_left", "anchor_right"), cols, dts)}
