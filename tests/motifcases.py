"""Shared by the tests of ``--genome`` / ``--strandFromMotif`` / ``--canonicalOnly``: the yardstick.  A restatement in Python of the
rule of ``include/spliser.h`` ("junction strand from the genome's splice motifs"), written from that text and without the product:
base codes, the FASTA rule, the motif code of a junction, the strand of a read, the tally; and the builders of the cases the tests
hold the product to.  Nothing here touches the GPU or the native library."""
import numpy as np

from spliser_amd import samio

COORD_MAX = 2 ** 31 - 67
_CODE = np.zeros(256, np.uint8)
for _letters, _c in (("Aa", 1), ("Cc", 2), ("Gg", 4), ("Tt", 8)):
    for _ch in _letters:
        _CODE[ord(_ch)] = _c
A, C, G, T = 1, 2, 4, 8
MOTIFS = {((G, T), (A, G)): 1, ((C, T), (A, C)): 2, ((G, C), (A, G)): 3, ((C, T), (G, C)): 4, ((A, T), (A, C)): 5, ((G, T), (A, T)): 6}
MOTIF_LETTERS = {1: ("GT", "AG"), 2: ("CT", "AC"), 3: ("GC", "AG"), 4: ("CT", "GC"), 5: ("AT", "AC"), 6: ("GT", "AT")}
REF_OPS = (0, 2, 3, 7, 8)     # M, D, N, =, X: the ops that move along the reference


class FastaError(Exception):
    def __init__(self, line, reason):
        Exception.__init__(self, "line %d: %s" % (line, reason))
        self.line, self.reason = line, reason


def parse_fasta(data):
    """bytes -> [(name bytes, codes uint8[length])]; ``FastaError(line, reason)`` with the 1-based line."""
    data = bytes(data)
    if data[:2] == b"\x1f\x8b":
        raise FastaError(1, "gzip")
    out, names, n_line = [], set(), 0
    pieces = data.split(b"\n")
    has_newline = [True] * (len(pieces) - 1) + [False]
    if pieces[-1] == b"":       # (the text ends with its last line's newline: nothing stands behind it)
        pieces.pop()
        has_newline.pop()
    for text, nl in zip(pieces, has_newline):
        n_line += 1
        if nl and text.endswith(b"\r"):
            text = text[:-1]
        if not text:
            continue
        if text[:1] == b">":
            name = text[1:]
            for stop in (b" ", b"\t", b"\r"):
                name = name.split(stop)[0]
            if not name:
                raise FastaError(n_line, "empty name")
            if name in names:
                raise FastaError(n_line, "repeated name")
            names.add(name)
            out.append((name, []))
        else:
            if not out:
                raise FastaError(n_line, "bytes before the first header")
            out[-1][1].append(_CODE[np.frombuffer(text, np.uint8)])
    if not out:
        raise FastaError(max(n_line, 1), "no sequence")
    return [(name, np.concatenate(parts) if parts else np.zeros(0, np.uint8)) for name, parts in out]


def motif_code(seq, left, right):
    """-> (code, outside): ``seq`` the codes of the sequence, base p at seq[p - 1]."""
    if right - left < 4:
        return 0, False
    if left + 1 < 1 or right > len(seq):
        return 0, True
    donor = (int(seq[left]), int(seq[left + 1]))            # bases left + 1, left + 2
    acceptor = (int(seq[right - 2]), int(seq[right - 1]))    # bases right - 1, right
    return MOTIFS.get((donor, acceptor), 0), False


def junctions_of(pos, ops):
    """Every N op of a read placed at ``pos`` -> [(left, right)]; the walk ends where an op would pass COORD_MAX."""
    cur, out = pos, []
    for op in ops:
        code, d = int(op) & 15, int(op) >> 4
        if code not in REF_OPS:
            continue
        if cur + d > COORD_MAX:
            break
        if code == 3:
            out.append((cur - 1, cur + d - 1))
        cur += d
    return out


def read_strand(flag, pos, ops, seq):
    """-> (byte, [code of every walk], outside): the read's strand byte, 43, 45 or 0."""
    if flag & 4 or pos < 1 or pos > COORD_MAX or len(ops) == 0:
        return 0, [], False
    codes, outside = [], False
    for l, r in junctions_of(pos, ops):
        c, o = motif_code(seq, l, r)
        codes.append(c)
        outside = outside or o
    plus, minus = any(c % 2 == 1 for c in codes), any(c and c % 2 == 0 for c in codes)
    return (43 if plus and not minus else 45 if minus and not plus else 0), codes, outside


def expected(rs, seq, shift=0):
    """-> (strand bytes uint8[n], tally int64[12]) for a ReadSet over one sequence: walks by code 0..6, reads +, -, conflicting,
    spliced without a canonical junction, with a pair outside."""
    out, tally = np.zeros(rs.n, np.uint8), np.zeros(12, np.int64)
    off = rs.cig_off.astype(np.int64)
    for i in range(rs.n):
        byte, codes, outside = read_strand(int(rs.flag[i]), int(rs.pos[i]) + shift, rs.cigar[off[i]:off[i + 1]], seq)
        out[i] = byte
        for c in codes:
            tally[c] += 1
        if codes:
            signs = {1 if c % 2 else -1 for c in codes if c}
            tally[7 if signs == {1} else 8 if signs == {-1} else 9 if len(signs) == 2 else 10] += 1
        tally[11] += 1 if outside else 0
    return out, tally


def table_by_strand(rs, bytes_, shift=0):
    """The mode-3 junction table the strand bytes imply: {(left, right, strand byte or '?'): supporting reads}, from the walk above."""
    rows, off = {}, rs.cig_off.astype(np.int64)
    for i in range(rs.n):
        if rs.flag[i] & 4 or rs.pos[i] < 0:
            continue
        for l, r in junctions_of(int(rs.pos[i]) + shift, rs.cigar[off[i]:off[i + 1]]):
            key = (l, r, int(bytes_[i]) or 63)
            rows[key] = rows.get(key, 0) + 1
    return rows


def expected_xs_tags(rs, seq):
    """The aux area (``XS:A`` or nothing) the rule gives every read, for ``samio.write_bam(tags=...)``."""
    return [b"XSA+" if b == 43 else b"XSA-" if b == 45 else b"" for b in expected(rs, seq)[0]]


# ---- builders --------------------------------------------------------------------------------------------------------------------
_LETTERS = np.frombuffer(b"ACGTACGTACGTacgtNnRYKMSWrykmBDHVbdhvU*-", np.uint8)


def random_bases(rng, n, plain=False):
    src = np.frombuffer(b"ACGT", np.uint8) if plain else _LETTERS
    return src[rng.integers(0, len(src), n)].tobytes()


def fasta_text(seqs, width=60, eol=b"\n"):
    out = []
    for name, bases in seqs:
        out.append(b">" + name + eol)
        out.extend(bases[k:k + width] + eol for k in range(0, len(bases), width))
    return b"".join(out)


CHUNK = 16384


def pack_corpus(seed=7):
    """One FASTA of under 1 MB with everything the pack must get right -> bytes (tests/test_gpu_motif.py names the parts)."""
    rng = np.random.default_rng(seed)
    t = bytearray()

    def line_ending_at(end):          # a sequence line whose newline is byte end - 1 of the file
        n = end - 1 - len(t)
        assert n > 0
        t.extend(random_bases(rng, n) + b"\n")

    def next_edge(room=200):
        return (len(t) + room + CHUNK - 1) // CHUNK * CHUNK

    t.extend(b"\n\n>first some description\n")                    # empty lines in front of the first header
    for k in range(12):
        t.extend(random_bases(rng, 60) + b"\n")
    line_ending_at(next_edge())                                    # ends exactly on a chunk edge
    t.extend(random_bases(rng, 7) + b"\n")
    line_ending_at(next_edge() - 1)                                # ... one byte in front of it
    t.extend(random_bases(rng, 33) + b"\n")
    line_ending_at(next_edge() + 1)                                # ... one byte behind it
    line_ending_at(next_edge() - 6)
    t.extend(b">header_across_a_chunk_edge\twith a tab and words behind it\n")
    t.extend(random_bases(rng, 61) + b"\n")
    t.extend(b">one_base_lines\n" + b"".join(bytes([b]) + b"\n" for b in random_bases(rng, 97)))
    t.extend(b">long_line\n" + random_bases(rng, 40000) + b"\n")    # a line longer than a chunk
    for n in (0, 1, 31, 32, 33, 63, 64, 65, 2, 30):                   # around one lane's store; odd and even
        t.extend(b">len%d\n" % n + (random_bases(rng, n) + b"\n" if n else b""))
    t.extend(b">crlf extra\r\n" + b"".join(random_bases(rng, 50) + b"\r\n" for _ in range(9)) + random_bases(rng, 13) + b"\r\n")
    t.extend(b">crlf_name_only\r\n" + b"\r\n" + random_bases(rng, 5) + b"\r\n\n\n")
    t.extend(b">lower\n" + random_bases(rng, 300).lower() + b"\n")
    t.extend(b">iupac\nNNNNNNNNNNRYKMSWBDHVnnnnACGTUu**--acgt\n")
    t.extend(b">ragged\n" + b"".join(random_bases(rng, int(n)) + b"\n" for n in rng.integers(1, 200, 300)))
    while t.count(b">") < 69:                                        # more headers than one wave has lanes
        k = t.count(b">")
        t.extend(b">filler%d\n" % k + fasta_text([(b"x", random_bases(rng, int(rng.integers(0, 5000))))], width=int(rng.integers(1, 120)))[3:])
    # windows of 64 KiB cut the big sequence's lines, and its CRLF pairs
    t.extend(b">big_crlf\r\n" + b"".join(random_bases(rng, 70) + b"\r\n" for _ in range(4000)))
    t.extend(b">last_without_newline\n" + random_bases(rng, 45) + b"\n" + random_bases(rng, 17))
    assert len(t) < 1000000 and t.count(b">") >= 70
    return bytes(t)


def window_cuts(text, window):
    """Where ``spl_genome_open`` cuts the text into windows of whole lines (include/spliser.h): a window ends behind the last newline
    among its first ``window`` bytes, or behind the line's own newline where that line is longer -> [file offset of every cut]."""
    cuts, lo = [], 0
    while lo < len(text):
        hi = min(len(text), lo + window)
        if hi < len(text):
            nl = text.rfind(b"\n", lo, hi)
            if nl < 0:
                nl = text.find(b"\n", hi)
            hi = nl + 1 if nl >= 0 else len(text)
        if hi < len(text):
            cuts.append(hi)
        lo = hi
    return cuts


def sequences_joined_across(text, window):
    """The cuts of ``window_cuts`` that fall inside a sequence -> [(cut, the sequence's bases in front of it)]: behind the cut the
    sequence goes on with a line of bases."""
    out = []
    for cut in window_cuts(text, window):
        rest = text[cut:].lstrip(b"\r\n")
        if rest[:1] in (b">", b""):
            continue
        out.append((cut, len(parse_fasta(text[:cut])[-1][1])))
    return out


def format_errors():
    """[(text, line, words of the reason)]: the four format errors, small and behind 200 kB of good text (a later window)."""
    rng = np.random.default_rng(3)
    good = fasta_text([(b"good", random_bases(rng, 200000))])
    n_good = good.count(b"\n")
    small = [(b"\nACGT\n>a\nAC\n", 2, "before the first"), (b">a\nAC\n> b\nAC\n", 3, "without a name"), (b">a\nAC\n>b\nA\n>a x\nC\n", 5, "second time"),
             (b"\n\r\n\n", 3, "no sequence")]
    return small + [(good + text, line + n_good, why) for text, line, why in small[1:3]]


def plant(seq, left, right, code):
    """The letters of motif ``code`` at junction (left, right) of a bytearray of bases."""
    donor, acceptor = MOTIF_LETTERS[code]
    seq[left:left + 2] = donor.encode()
    seq[right - 2:right] = acceptor.encode()


def planted_case():
    """-> (bases bytes, ReadSet, [(left, right)]): hand-built reads over a sequence that has the motifs planted where the kernel can
    go wrong (tests/test_gpu_motif.py lists them)."""
    rng = np.random.default_rng(11)
    # (T-free background: no pair of the background is a donor or acceptor of the six by accident -- every one of them holds a T
    #  or is AG / AC / GC, which "AAAA.." and "CCCC.." stretches below avoid where it matters; the yardstick decides anyway)
    seq = bytearray(random_bases(rng, 20000, plain=True))
    recs, juncs = [], []

    def read(flag, pos, cigar):
        recs.append((flag, pos, cigar))

    def one(left, length, code=None, anchor=20):
        right = left + length
        if code:
            plant(seq, left, right, code)
        juncs.append((left, right))
        read(0, left - anchor + 1, "%dM%dN%dM" % (anchor, length, anchor))
        return right

    at = 100
    for code in range(1, 7):                                   # each motif, donor pair at an even and at an odd position
        for parity in (0, 1):
            left = at + (at + parity) % 2
            one(left, 80 + code, code)
            at += 300
    one(32 * 120 + 31, 70, 1)                                  # the donor pair across a 16-byte word of the store (bases 32 k, 32 k + 1)
    one(32 * 130 + 1 - 70, 70, 2)                              # ... the acceptor pair across one
    one(32 * 140 + 15, 64, 5)                                  # an odd left: both pairs across a byte
    one(32 * 150 + 16, 64, 6)                                  # an even one: each pair in one byte
    for length in (1, 2, 3, 4, 5):                                # introns of length 1 to 5: GTAG in four bases is code 1
        left = 8000 + 100 * length
        seq[left:left + 6] = b"GTAGAG" if length != 5 else b"GTCAGA"
        juncs.append((left, left + length))
        read(16, left - 9, "10M%dN10M" % length)
    for k, (d, a) in enumerate((("NT", "AG"), ("GN", "AG"), ("GT", "NG"), ("GT", "An"))):   # an N in either pair
        left = 9000 + 100 * k
        seq[left:left + 2], seq[left + 48:left + 50] = d.encode(), a.encode()
        juncs.append((left, left + 50))
        read(0, left - 4, "5M50N5M")
    # the sequence's first and last possible positions: an N op as the first op, and one that ends on the last base
    plant(seq, 0, 40, 3)
    juncs.append((0, 40))
    read(0, 1, "40N20M")
    plant(seq, len(seq) - 50, len(seq), 6)
    juncs.append((len(seq) - 50, len(seq)))
    read(0, len(seq) - 59, "10M50N")
    read(0, len(seq) - 59, "10M51N5M")                          # ... and one base beyond it: outside
    read(0, len(seq) - 5, "5M30N5M")
    # two junctions: agreeing, conflicting, one canonical and one code 0; a read of 70 N ops; no N; unmapped; unplaced
    base = 10000
    for k, code in enumerate((1, 3, 2, 4, 5, 6, 1, 0, 0, 2)):
        left = base + 100 * k
        if code:
            plant(seq, left, left + 50, code)
        else:
            seq[left:left + 2] = b"AA"
        juncs.append((left, left + 50))
    two = lambda k, flag=0: read(flag, base + 100 * k - 9, "10M50N50M50N10M")
    two(0); two(2); two(4, 16)      # +,+   -,-   +,-
    two(1); two(3); two(5)          # +,-   -,+   -,+
    two(6); two(7); two(8)          # +,0   0,0   0,-
    for k in range(70):
        plant(seq, 12000 + 40 * k + 10, 12000 + 40 * k + 40, 1 if k != 69 else 2)
    read(0, 12001, "10M30N" * 70 + "5M")
    read(0, 12001, "10M30N" * 69 + "5M")
    for pos in (50, 5000, 19900):
        read(0, pos, "60M")
        read(16, pos, "5S20M2I20M3D10M")
    read(4, 109, "20M81N20M")
    read(4 | 16, 109, "20M81N20M")
    read(0, 0, "20M81N20M")
    read(0, -7, "20M81N20M")
    read(0, 300, "*")
    rs = samio.ReadSet.from_records([(f, p, c) for f, p, c in recs if c != "*"])
    return bytes(seq), rs, juncs


def random_case(seed, n_reads, length=50000, n_junctions=90):
    """-> (bases bytes, ReadSet, [(left, right)]): a random sequence with a catalogue of junctions, a third of them '+', a third '-', a
    third without a canonical motif, and random reads over them: unspliced, one junction, two neighbouring ones."""
    rng = np.random.default_rng(seed)
    seq = bytearray(random_bases(rng, length))
    step = length // (n_junctions + 2)
    juncs = []
    for k in range(n_junctions):
        left = step * (k + 1) + int(rng.integers(0, 40))
        right = left + int(rng.integers(70, step - 120))
        code = int(rng.integers(0, 9))
        if 1 <= code <= 6:
            plant(seq, left, right, code)
        juncs.append((left, right))
    recs = []
    for _ in range(n_reads):
        kind = rng.random()
        flag = int(rng.choice([0, 16, 99, 147, 256, 4], p=[.4, .4, .07, .07, .04, .02]))
        if kind < 0.45:
            recs.append((flag, int(rng.integers(1, length - 200)), "%dM" % int(rng.integers(30, 150))))
            continue
        k = int(rng.integers(0, n_junctions - 1))
        a, b = int(rng.integers(1, 60)), int(rng.integers(1, 60))
        (l0, r0), (l1, r1) = juncs[k], juncs[k + 1]
        cigar = "%dM%dN" % (a, r0 - l0)
        if kind < 0.7:
            cigar += "%dM" % b
        else:
            cigar += "%dM%dN%dM" % (l1 - r0, r1 - l1, b)
        if rng.random() < 0.15:
            cigar = "%dS" % int(rng.integers(1, 9)) + cigar
        recs.append((flag, l0 - a + 1, cigar))
    recs.sort(key=lambda r: r[1])
    return bytes(seq), samio.ReadSet.from_records(recs), juncs


def codes_of(bases):
    return _CODE[np.frombuffer(bytes(bases), np.uint8)]
