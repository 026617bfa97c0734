"""DEFLATE streams written by hand to land on the limits of the device inflate (spliser_amd/csrc/spl_inflate_wave.h: decode_block,
build_lut, decode, count_from / emit_from, copy_block): a bit-level writer that takes code lengths, header fields and the run-length
spelling of a dynamic header as GIVEN, a plain RFC 1951 reader (bit by bit, canonical codes by counting, no tables) and the named
cases.  Shared by test_deflate_cases_host.py (CPU: the cases are what they say; the kernel body under the wave emulator) and
test_gpu_inflate_limits.py (the same cases through the launchers on the card).  zlib's compressor writes a narrow family of streams;
other BAM writers (libdeflate, zlib-ng, ISA-L) have other habits, and RFC 1951 allows far more than any of them writes.

What a case expects -- the policy:
  legal    zlib.decompress takes the stream: status 0 and zlib's bytes.
  refuse   zlib refuses it AND decoding it would make wrong bytes, an out-of-range copy or an out-of-range table: the status is not
           0; where the case names a code, it is that code.
  lenient  zlib refuses it, but only for a code that is incomplete while none of its missing codes is used: either a status that is
           not 0, or status 0 with exactly the plain reader's bytes.
  always   nothing is written behind the block's output or behind its token room; the other blocks of the launch are untouched.

The constants come from the kernel sources, as in limitcases.py and junctioncases.py, so the cases follow the code when it is retuned."""
import os
import re
import zlib
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spliser_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _one(pattern, text):
    found = set(re.findall(pattern, text, re.M))
    assert len(found) == 1, (pattern, found)
    return found.pop()


_WAVE, _HEAD = _source("spl_inflate_wave.h"), _source("spl_inflate.h")


def _wave_constant(name):
    v = _one(r"\b%s = (\w+?)u?[,;]" % name, _WAVE)
    if not v.isdigit():                                 # (an #ifndef default: constexpr uint32_t RING = SPLZ_RING;)
        v = _one(r"^#define %s (\d+)\s*$" % v, _WAVE)
    return int(v)


ROOT_L, ROOT_D, ROOT_C = (_wave_constant(n) for n in ("ROOT_L", "ROOT_D", "ROOT_C"))
LUT_L, LUT_D = _wave_constant("LUT_L"), _wave_constant("LUT_D")
SUB_BITS, TILE_PAD = _wave_constant("SUB_BITS"), _wave_constant("TILE_PAD")
TOKCAP, TOKCAP_SMALL = _wave_constant("TOKCAP"), _wave_constant("TOKCAP_SMALL")
RING, FIFO, BEAT = _wave_constant("RING"), _wave_constant("FIFO"), _wave_constant("BEAT")
Z = {name: int(v) for name, v in re.findall(r"^#define (SPL_Z_[A-Z_0-9]+) (\d+)u", _HEAD, re.M)}
SPL_Z_TOKEN_STRIDE, SPL_Z_IMAGE_PAD = Z["SPL_Z_TOKEN_STRIDE"], Z["SPL_Z_IMAGE_PAD"]
OK, BAD_BLOCK_TYPE, BAD_STORED, BAD_LENGTHS, BAD_CODE = (Z["SPL_Z_" + n] for n in ("OK", "BAD_BLOCK_TYPE", "BAD_STORED", "BAD_LENGTHS", "BAD_CODE"))
BAD_DISTANCE, OVERRUN, SHORT, BAD_CRC, TOKENS = (Z["SPL_Z_" + n] for n in ("BAD_DISTANCE", "OVERRUN", "SHORT", "BAD_CRC", "TOKENS"))
TILE_BITS = 64 * SUB_BITS

# RFC 1951, 3.2.5 and 3.2.7
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class _Bits:
    """DEFLATE's bit order: fields LSB first, Huffman codes MSB first (RFC 1951 3.1.1)."""

    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, bits):
        self.acc |= value << self.n
        self.n += bits
        while self.n >= 8:
            self.buf.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, bits):
        self.put(int(format(value, "0%db" % bits)[::-1], 2), bits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def _mixed_block(n_pairs, n_stored, seed=5):
    """One DEFLATE stream: a fixed-code section of `n_pairs` x (lone literal, match of length 3 at distance 1) -- 5 bytes of
    tokens for 4 of output, the most a Huffman section can ask for -- then `n_stored` stored sections of ONE byte each (2 bytes of
    tokens per byte of output).  -> (data, comp)"""
    rng = np.random.default_rng(seed)
    w, data = _Bits(), bytearray()
    w.put(0, 1), w.put(1, 2)                        # not the last section, fixed code
    for lit in rng.integers(0, 144, n_pairs):
        w.code(0x30 + int(lit), 8)                  # literal 0..143: 8 bits, 00110000 + value
        w.code(1, 7)                                # 257 = length 3: 7 bits, 0000001
        w.code(0, 5)                                # distance code 0 = 1
        data += bytes([int(lit)]) * 4
    w.code(0, 7)                                    # 256, the section's end
    for k, b in enumerate(rng.integers(0, 256, n_stored)):
        w.put(1 if k == n_stored - 1 else 0, 1), w.put(0, 2)
        w.align()
        w.put(1, 16), w.put(0xfffe, 16), w.put(int(b), 8)
        data.append(int(b))
    w.align()
    comp = bytes(w.buf)
    assert zlib.decompress(comp, -15) == bytes(data)
    return bytes(data), comp


def canonical(lens):
    """code lengths -> {symbol: (code, bits)}, the canonical assignment of RFC 1951 3.2.2 (codes of an over-subscribed set overflow
    their length: the writer masks them, the stream is damaged on purpose)"""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n] & ((1 << n) - 1), n)
            nxt[n] += 1
    return out


def flat_lens(n_used):
    """lengths of a COMPLETE code over n_used >= 2 symbols: some of k - 1 bits, the rest of k"""
    k = max(1, (n_used - 1).bit_length())
    short = (1 << k) - n_used
    return [k - 1] * short + [k] * (n_used - short)


def length_symbol(length):
    return 285 if length == 258 else 257 + max(i for i in range(28) if LEN_BASE[i] <= length)


def distance_symbol(dist):
    return max(i for i in range(30) if DIST_BASE[i] <= dist)


def expand_rle(rle):
    """the run-length spelling of a dynamic header -> the lengths it says (None where it is not sayable: 16 with nothing before)"""
    out = []
    for item in rle:
        if isinstance(item, int):
            out.append(item)
        elif item[0] == 16:
            if not out:
                return None
            out += [out[-1]] * item[1]
        else:
            out += [0] * item[1]
    return out


class Writer(_Bits):
    """Sections of a DEFLATE stream from symbols: an int is a literal (or 256, or a length symbol put down bare), a tuple is
    (length, distance[, length symbol[, distance symbol]]).  `out` is what the stream inflates to, `too_far` whether a match reached
    back past the first byte (its bytes are then zeros here)."""

    def __init__(self):
        super().__init__()
        self.out, self.too_far = bytearray(), False

    @property
    def pos(self):
        return len(self.buf) * 8 + self.n

    def symbols(self, syms, lit, dist):
        for s in syms:
            if isinstance(s, (int, np.integer)):
                self.code(*lit[int(s)])
                if s < 256:
                    self.out.append(int(s))
                continue
            length, d = s[0], s[1]
            ls = s[2] if len(s) > 2 else length_symbol(length)
            ds = s[3] if len(s) > 3 else distance_symbol(d)
            self.code(*lit[ls])
            self.put(length - LEN_BASE[ls - 257], LEN_EXTRA[ls - 257])
            self.code(*dist[ds])
            if ds < 30:
                self.put(d - DIST_BASE[ds], DIST_EXTRA[ds])
            else:
                self.put(0, 14)                        # (what the arithmetic of symbols 28 and 29, carried on, would take for extra bits)
            if d > len(self.out):
                self.too_far = True
                self.out[:0] = bytes(d - len(self.out))
            for _ in range(length):
                self.out.append(self.out[-d])

    def stored(self, data, last=0, nlen=None):
        self.put(last, 1), self.put(0, 2)
        self.align()
        self.put(len(data), 16), self.put((len(data) ^ 0xffff) if nlen is None else nlen, 16)
        for b in data:
            self.put(b, 8)
        self.out += data

    def fixed(self, syms, last=0, eob=True):
        self.put(last, 1), self.put(1, 2)
        self.symbols(list(syms) + ([256] if eob else []), canonical(FIXED_LIT), canonical(FIXED_DIST))

    def dynamic_header(self, lit_lens, dist_lens, last=0, rle=None, cl_lens=None, hclen=15, hlit=None, hdist=None, cut=None):
        """cut: stop after this many header fields (0 = after the three bits of the section's head, 1 = HLIT, 2 = HDIST, 3 = HCLEN,
        4 = half the code-length code's lengths, 5 = all of them, 6 = half the lengths)"""
        self.put(last, 1), self.put(2, 2)
        if rle is None:
            rle = list(lit_lens) + list(dist_lens)
        if cl_lens is None:
            used = sorted({item if isinstance(item, int) else item[0] for item in rle})
            if len(used) == 1:
                used.append(0 if used[0] else 1)
            cl_lens = [0] * 19
            for s, n in zip(used, flat_lens(len(used))):
                cl_lens[s] = n
        fields = [(len(lit_lens) - 257 if hlit is None else hlit, 5), (len(dist_lens) - 1 if hdist is None else hdist, 5), (hclen, 4)]
        for k, (v, bits) in enumerate(fields):
            if cut is not None and cut <= k:
                return
            self.put(v, bits)
        n_code = hclen + 4
        for k in range(n_code):
            if cut == 4 and k == n_code // 2:
                return
            self.put(cl_lens[CLEN_ORDER[k]], 3)
        if cut == 5:
            return
        assert all(cl_lens[CLEN_ORDER[k]] == 0 for k in range(n_code, 19)), "HCLEN leaves out a length that is used"
        cl = canonical(cl_lens)
        for k, item in enumerate(rle):
            if cut == 6 and k == len(rle) // 2:
                return
            if isinstance(item, int):
                self.code(*cl[item])
            else:
                self.code(*cl[item[0]])
                self.put(item[1] - (11 if item[0] == 18 else 3), {16: 2, 17: 3, 18: 7}[item[0]])

    def dynamic(self, syms, lit_lens, dist_lens, last=0, eob=True, **header):
        self.dynamic_header(lit_lens, dist_lens, last, **header)
        self.symbols(list(syms) + ([256] if eob else []), canonical(lit_lens), canonical(dist_lens))

    def done(self):
        self.align()
        return bytes(self.buf)


# ---- the plain reader ----------------------------------------------------------------------------------------------------------

class Refused(ValueError):
    pass


class _Reader:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def bits(self, n):
        v = 0
        for k in range(n):
            if self.pos >= 8 * len(self.data):
                raise Refused("the stream ends early")
            v |= ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1) << k
            self.pos += 1
        return v


def _counted(lens, what):
    """code lengths -> (count per length, symbols in canonical order); over-subscribed sets are refused, incomplete ones are not"""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    left = 1
    for bits in range(1, 16):
        left = (left << 1) - count[bits]
        if left < 0:
            raise Refused("over-subscribed %s code" % what)
    return count, [s for bits in range(1, 16) for s, n in enumerate(lens) if n == bits]


def _symbol(rd, code):
    count, symbols = code
    c = first = index = 0
    for bits in range(1, 16):
        c |= rd.bits(1)
        if c - count[bits] < first:
            return symbols[index + c - first]
        index += count[bits]
        first = (first + count[bits]) << 1
        c <<= 1
    raise Refused("no such code")


def inflate(comp, limit=1 << 17):
    """RFC 1951, read the slow and obvious way.  Lenient in ONE respect: a code that is incomplete is taken as long as no missing
    code turns up (zlib refuses such a header outright, except for a lone distance code of one bit)."""
    rd, out = _Reader(comp), bytearray()
    last = 0
    while not last:
        last, kind = rd.bits(1), rd.bits(2)
        if kind == 3:
            raise Refused("block type 3")
        if kind == 0:
            rd.pos = (rd.pos + 7) & ~7
            n, nn = rd.bits(16), rd.bits(16)
            if n ^ 0xffff != nn:
                raise Refused("stored: NLEN")
            for _ in range(n):
                out.append(rd.bits(8))
            continue
        if kind == 1:
            lit, dist = _counted(FIXED_LIT, "literal"), _counted(FIXED_DIST, "distance")
        else:
            n_lit, n_dist, n_code = rd.bits(5) + 257, rd.bits(5) + 1, rd.bits(4) + 4
            if n_lit > 286 or n_dist > 30:
                raise Refused("too many symbols")
            cl = [0] * 19
            for k in range(n_code):
                cl[CLEN_ORDER[k]] = rd.bits(3)
            clc = _counted(cl, "code-length")
            lens = []
            while len(lens) < n_lit + n_dist:
                s = _symbol(rd, clc)
                if s < 16:
                    lens.append(s)
                    continue
                if s == 16:
                    if not lens:
                        raise Refused("16 first")
                    prev, rep = lens[-1], 3 + rd.bits(2)
                else:
                    prev, rep = 0, (3 + rd.bits(3)) if s == 17 else (11 + rd.bits(7))
                if len(lens) + rep > n_lit + n_dist:
                    raise Refused("a run past the last length")
                lens += [prev] * rep
            if lens[256] == 0:
                raise Refused("no end-of-block code")
            lit, dist = _counted(lens[:n_lit], "literal"), _counted(lens[n_lit:], "distance")
        while True:
            s = _symbol(rd, lit)
            if s < 256:
                out.append(s)
            elif s == 256:
                break
            else:
                if s > 285:
                    raise Refused("length symbol %d" % s)
                length = LEN_BASE[s - 257] + rd.bits(LEN_EXTRA[s - 257])
                ds = _symbol(rd, dist)
                if ds > 29:
                    raise Refused("distance symbol %d" % ds)
                d = DIST_BASE[ds] + rd.bits(DIST_EXTRA[ds])
                if d > len(out):
                    raise Refused("distance too far back")
                for _ in range(length):
                    out.append(out[-d])
            if len(out) > limit:
                raise Refused("too long")
    return bytes(out)


def zlib_takes(comp):
    try:
        d = zlib.decompressobj(-15)
        data = d.decompress(comp)
        return data if d.eof else None
    except zlib.error:
        return None


# ---- the sizing rule of build_lut, restated ------------------------------------------------------------------------------------

def table_entries(lens, root):
    """Entries of the two-level table of a canonical code: 1 << root for the root table, and one sub-table for every root prefix
    that codes longer than `root` begin with, 1 << (the longest such code - root)."""
    longest = {}
    for s, (code, bits) in canonical(lens).items():
        if bits > root:
            p = code >> (bits - root)
            longest[p] = max(longest.get(p, 0), bits - root)
    return (1 << root) + sum(1 << b for b in longest.values())


def _spread(counts, n):
    """{length: how many} -> lengths of symbols 0..n-1, ascending (unused symbols: 0)"""
    lens = [bits for bits in sorted(counts) for _ in range(counts[bits])]
    assert len(lens) <= n
    return lens + [0] * (n - len(lens))


# Found once, offline, by an exhaustive search over the complete codes of (286 symbols, 15 bits) and (30 symbols, 15 bits) -- memoised
# on (length, free codes of that length, symbols left, longest code in the open root prefix); what matters is how many codes have
# each length, canonical codes being assigned in order of length.  Both reach the tables' sizes (zlib's ENOUGH values).
LIT_MOST = ({2: 3, 10: 233, 11: 45, 12: 1, 13: 1, 14: 1, 15: 2}, 852)
DIST_MOST = ({2: 3, 3: 1, 7: 13, 8: 5, 9: 1, 10: 1, 11: 1, 12: 1, 13: 1, 14: 1, 15: 2}, 592)
# INCOMPLETE codes that need more than the tables have (a lone 1-bit code leaves half the code space to long codes): by hand
LIT_OVER = ({1: 1, 10: 279, 11: 1, 12: 1, 13: 1, 14: 1, 15: 2}, 854)
DIST_OVER = ({1: 1, 7: 21, 8: 1, 9: 1, 10: 1, 11: 1, 12: 1, 13: 1, 14: 1, 15: 1}, 596)

# Every code length 1..15 in one code (two of 15 bits): sub-tables of every width up to 15 - root, the widest there is.
# a, b: literals of one and two bits (a stream can be padded to any bit); c: a literal of the sub-table; d: of the root table's last
# length; 257 in 8 bits and distance symbol 0 in 8: a match of 16 bits, sixteen to a lane; 284 and distance symbol 29 in 15 bits:
# with their 5 and 13 extra bits the longest symbol DEFLATE has, 48 bits.
A, B, C_, D_ = 0x61, 0x62, 0x63, 0x64
_COMB_L = {A: 1, B: 2, 256: 3, 258: 4, 285: 5, 0x65: 6, 0x66: 7, 257: 8, D_: 9, C_: 10, 0x67: 11, 0x68: 12, 0x69: 13, 0x6a: 14, 284: 15, 283: 15}
_COMB_D = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 7, 0: 8, 8: 9, 9: 10, 10: 11, 11: 12, 12: 13, 13: 14, 28: 15, 29: 15}
COMB_LIT = [_COMB_L.get(s, 0) for s in range(286)]
COMB_DIST = [_COMB_D.get(s, 0) for s in range(30)]
FILL = (3, 1)                                          # the 16-bit match of the comb code

Case = namedtuple("Case", "name limit kind comp data code info")


def _case(name, limit, w, kind="legal", code=None, data=None, **info):
    comp = w.done() if isinstance(w, Writer) else w
    if data is None:
        data = bytes(w.out) if isinstance(w, Writer) else b""
    if kind != "legal" and not data:
        data = b"\0"                                   # (a block of no bytes is never decoded: give the refusals something to make)
    assert len(comp) <= 65536 and len(data) <= 65536, name
    return Case(name, limit, kind, comp, data, code, info)


def _lits(rng, n, hi=256):
    return [int(v) for v in rng.integers(0, hi, n)]


# ---- dynamic headers -----------------------------------------------------------------------------------------------------------

def header_cases():
    rng = np.random.default_rng(101)
    out = []
    flat8 = [8] * 255 + [0] + [8]                      # literals 0..254 and 256 in 8 bits: complete, and sayable with 0 and 8 alone

    def small(n_lit=258, n_dist=1):
        lit = [0] * n_lit
        for s, n in zip((0x41, 0x42, 256, 257), (1, 2, 3, 3) if n_lit > 257 else (1, 2, 2)):
            lit[s] = n
        dist = [0] * n_dist
        dist[0] = 1
        return lit, dist
    body = [0x41, 0x42, 0x41, (3, 1), 0x42, 0x41]
    for hlit in (0, 29):
        for hdist in (0, 29):
            w = Writer()
            lit, dist = small(257 + hlit, 1 + hdist)
            w.dynamic(body if hlit else [0x41, 0x42, 0x42, 0x41], lit, dist, last=1)
            out.append(_case("hlit%d_hdist%d" % (hlit, hdist), "HLIT = %d, HDIST = %d: the fewest and the most lengths a header lists" % (hlit, hdist), w))
    w = Writer()
    w.dynamic(_lits(rng, 300, 255), flat8, [0], last=1, hclen=1, rle=[8] * 255 + [0, 8, 0])
    out.append(_case("hclen1", "HCLEN = 1: five lengths of the code-length code (16, 17, 18, 0, 8), the fewest that can say a code with an end-of-block", w))
    w = Writer()
    w.dynamic_header([0] * 257, [0], last=1, hclen=0, cl_lens=[2 if s in (0, 16, 17, 18) else 0 for s in range(19)], rle=[0, (18, 138), (18, 119)])
    out.append(_case("hclen0", "HCLEN = 0: lengths of 16, 17, 18 and 0 alone can only say 'no code at all': no end-of-block", w, "refuse", BAD_LENGTHS))
    w = Writer()
    lit, dist = small()
    w.dynamic(body, lit, dist, last=1, hclen=15)
    out.append(_case("hclen15", "HCLEN = 15: all nineteen lengths of the code-length code", w))
    w = Writer()
    lit = [0] * 257
    lit[0x41], lit[256] = 1, 1
    w.dynamic([0x41] * 40, lit, [0], last=1)
    out.append(_case("dist_one_symbol_length0", "a distance code of one symbol with length 0: the block has no match at all", w))
    w = Writer()
    lit, dist = small()
    w.dynamic(body, lit, dist, last=1)
    out.append(_case("dist_one_symbol_length1", "a distance code of one symbol with length 1 (incomplete, and legal)", w))
    # symbol 16 repeats the LAST LITERAL length into the first distance lengths
    lit, dist = [0] * 260, [5] * 30
    for s in list(range(0, 22)) + list(range(250, 260)):
        lit[s] = 5
    dist[28] = dist[29] = 4                              # 32 codes of 5 bits for the literals and lengths; 28 x 1/32 + 2 x 1/16 = 1 for the distances
    w = Writer()
    rle = lit[:259] + [5, (16, 6), (16, 6), (16, 6), (16, 6), (16, 4), 4, 4]
    assert expand_rle(rle) == lit + dist
    w.dynamic([1, 2, 3, 250, (5, 2), 7, (4, 4)], lit, dist, last=1, rle=rle)
    out.append(_case("rep16_across_boundary", "symbol 16 repeats the last literal/length length into the first distance lengths", w))
    # a 17 run and an 18 run across the boundary
    lit, dist = [0] * 260, [0] * 12
    lit[0x41], lit[0x42], lit[256], lit[257] = 1, 2, 3, 3
    dist[10], dist[11] = 1, 1
    w = Writer()
    rle = lit[:257] + [3, (17, 10), 0, 0, 1, 1]
    assert expand_rle(rle) == lit + dist
    w.dynamic([0x41] * 60 + [0x42, (3, 33), (3, 49)], lit, dist, last=1, rle=rle)
    out.append(_case("run17_across_boundary", "a run of zeros (17) that begins in the literal lengths and ends in the distance lengths", w))
    lit, dist = [0] * 270, [0] * 30
    lit[0x41], lit[0x42], lit[256], lit[257] = 1, 2, 3, 3
    dist[28], dist[29] = 1, 1
    w = Writer()
    rle = lit[:258] + [(18, 12 + 28), 1, 1]
    assert expand_rle(rle) == lit + dist
    w.dynamic([0x41] * 40, lit, dist, last=1, rle=rle)
    out.append(_case("run18_across_boundary", "a run of zeros (18) that begins in the literal lengths and ends in the distance lengths", w))
    lit = [0] * 257
    lit[150], lit[151], lit[256] = 1, 2, 2
    w = Writer()
    rle = [(18, 138), (18, 12), 1, 2, (18, 104), 2, 0]
    assert expand_rle(rle) == lit + [0] and len(lit) == 257
    w.dynamic([150, 151, 150, 150], lit, [0], last=1, rle=rle)
    out.append(_case("run18_of_138", "an 18 run of 138 zeros, the longest there is (7 extra bits all ones)", w))
    # a code-length code that uses all of 7 bits: lengths 1, 2, .. 6, 7, 7
    cl = [0] * 19
    for s, n in zip((0, 8, 7, 9, 6, 18, 17, 16), (1, 2, 3, 4, 5, 6, 7, 7)):
        cl[s] = n
    lit = [8] * 64 + [7] * 32 + [9] * 128 + [0] * 32 + [6]
    for s in range(224, 239):
        lit[s] = 6                                      # 64/256 + 32/128 + 128/512 + 16/64 = 1
    assert sum(2.0 ** -n for n in lit if n) == 1.0
    w = Writer()
    rle = [8] * 64 + [7] * 32 + [9, (16, 6)] * 18 + [9, 9] + [6] * 15 + [(17, 3), (18, 14)] + [6, 0]
    assert expand_rle(rle) == lit + [0]
    w.dynamic(_lits(rng, 200, 224) + [230, 238, 224], lit, [0], last=1, rle=rle, cl_lens=cl)
    out.append(_case("clen_code_7_bits", "a code-length code whose longest codes have 7 bits, all the root table has", w))

    # ---- refusals that zlib shares
    lit, dist = small()
    for hlit in (30, 31):
        w = Writer()
        lit2 = [0] * (257 + hlit)
        for s, n in zip((0x41, 0x42, 256, 257), (1, 2, 3, 3)):
            lit2[s] = n
        w.dynamic(body, lit2, dist, last=1)
        out.append(_case("hlit%d" % hlit, "HLIT = %d: more literal/length lengths than there are symbols" % hlit, w, "refuse", BAD_LENGTHS))
    w = Writer()
    w.dynamic(body, lit, dist, last=1, rle=[(16, 3)] + lit[3:] + dist)
    out.append(_case("rep16_first", "symbol 16 as the first length: nothing to repeat", w, "refuse", BAD_LENGTHS))
    w = Writer()
    w.dynamic(body, lit, dist, last=1, rle=lit[:256] + [3, 3, (17, 3)])
    out.append(_case("run_past_the_end", "a run that goes past HLIT + HDIST lengths", w, "refuse", BAD_LENGTHS))
    w = Writer()
    no_eob = list(lit)
    no_eob[256], no_eob[0x43] = 0, 3
    w.dynamic([0x41, 0x42, 0x43], no_eob, dist, last=1, eob=False)
    out.append(_case("no_end_of_block", "a literal/length code without symbol 256", w, "refuse", BAD_LENGTHS))
    w = Writer()
    over = list(lit)
    over[0x43] = 1                                      # two codes of one bit and more
    w.dynamic(body, over, dist, last=1)
    out.append(_case("oversubscribed_literal", "an over-subscribed literal/length code", w, "refuse", BAD_LENGTHS))
    w = Writer()
    w.dynamic(body, lit, [1, 1, 1], last=1)
    out.append(_case("oversubscribed_distance", "an over-subscribed distance code", w, "refuse", BAD_LENGTHS))
    w = Writer()
    w.dynamic(body, lit, dist, last=1, cl_lens=[1 if s < 4 else 0 for s in range(19)])
    out.append(_case("oversubscribed_code_length", "an over-subscribed code-length code", w, "refuse", BAD_LENGTHS))
    w = Writer()
    w.put(1, 1), w.put(3, 2), w.put(0x5555, 16)
    out.append(_case("block_type_3", "block type 3", w, "refuse", BAD_BLOCK_TYPE))
    w = Writer()
    w.fixed([0x41] * 5)
    w.stored(b"hello", last=1, nlen=5 ^ 0xfffe)
    out.append(_case("stored_nlen", "a stored section whose NLEN is not the complement of LEN", w, "refuse", BAD_STORED))
    lit, dist = small(286, 30)
    for cut, what in enumerate(("the section's head", "HLIT", "HDIST", "HCLEN", "half the code-length code", "the code-length code", "half the lengths")):
        w = Writer()
        w.dynamic_header(lit, dist, last=1, cut=cut)
        comp = bytes(w.buf)                             # (whole bytes only: what is left in the accumulator is cut off as well)
        if cut == 0:
            comp = b""
        out.append(_case("header_cut_%d" % cut, "the block's data ends behind %s" % what, comp, "refuse", OVERRUN, data=b"AB"))
    # ---- what zlib refuses and a decoder may take: incomplete codes none of whose missing codes is used
    w = Writer()
    lit = [0] * 258
    lit[0x41], lit[0x42], lit[256], lit[257] = 2, 2, 2, 3   # 7/8 of the code space
    w.dynamic(body, lit, [2, 2], last=1)
    out.append(_case("incomplete_codes_unused", "incomplete literal/length and distance codes, the missing codes never used", w, "lenient"))
    w = Writer()
    w.dynamic_header(lit, [2, 2], last=1)
    w.symbols([0x41, 0x42], canonical(lit), canonical([2, 2]))
    w.code(7, 3), w.code(7, 3), w.code(7, 3)              # 111: a code nobody has
    out.append(_case("incomplete_code_used", "an incomplete literal/length code and the missing code in the data", w, "refuse", BAD_CODE, data=b"AB\0"))
    return out


# ---- table building ------------------------------------------------------------------------------------------------------------

def table_cases():
    rng = np.random.default_rng(102)
    out = []
    lit, dist = _spread(LIT_MOST[0], 286), _spread(DIST_MOST[0], 30)
    syms = []
    for k in range(400):                                # symbols of every length of both codes, matches at every distance symbol in reach
        syms.append(int(rng.choice([0, 1, 2, 3, 100, 235, 236, 255])))
        if k % 3 == 0 and k > 20:
            length = int(rng.choice([3, 4, 10, 130, 131, 162, 163, 194, 226, 227, 257, 258]))
            d = int(rng.integers(1, 1 + sum(1 for s in syms if isinstance(s, int)) // 2))
            syms.append((length, max(1, d)))
    w = Writer()
    w.dynamic(syms[:200], lit, dist)
    w.dynamic(syms[200:] + [(258, 1)] * 130 + [(258, 24577 + 8191, 284), (200, 24577), (4, 16385), (5, 12289)], lit, dist, last=1)
    out.append(_case("tables_full", "code lengths that need every entry of both tables: %d of LUT_L and %d of LUT_D" % (LIT_MOST[1], DIST_MOST[1]), w,
                     lit=lit, dist=dist))
    w = Writer()
    w.dynamic([1, 2, 3], _spread(LIT_OVER[0], 286), [1, 1], last=1)
    out.append(_case("literal_table_over", "an incomplete literal/length code that needs %d entries, more than LUT_L" % LIT_OVER[1], w, "refuse", BAD_LENGTHS, reader_takes=True))
    w = Writer()
    lit = [0] * 257
    lit[1], lit[2], lit[3], lit[256] = 2, 2, 2, 2
    w.dynamic([1, 2, 3], lit, _spread(DIST_OVER[0], 30), last=1)
    out.append(_case("distance_table_over", "an incomplete distance code that needs %d entries, more than LUT_D" % DIST_OVER[1], w, "refuse", BAD_LENGTHS, reader_takes=True))
    # the fixed code has codes for 286, 287 and distance symbols 30, 31: present, and an error when used
    w = Writer()
    w.fixed(_lits(rng, 50) + [(10, 7), (3, 50)], last=1)
    out.append(_case("fixed_unused_symbols", "the fixed code: codes for 286 / 287 and distance symbols 30 / 31 are there, unused", w))
    for s in (286, 287):
        w = Writer()
        w.put(1, 1), w.put(1, 2)
        w.symbols([1, 2, 3, s, 4, 256], canonical(FIXED_LIT), canonical(FIXED_DIST))
        out.append(_case("fixed_symbol_%d" % s, "length symbol %d of the fixed code in the data" % s, w, "refuse", BAD_CODE, data=b"\1\2\3\4"))
    for s in (30, 31):
        w = Writer()
        w.put(1, 1), w.put(1, 2)
        w.symbols(list(range(40)) + [(3, 1, 257, s), 4, 256], canonical(FIXED_LIT), canonical(FIXED_DIST))
        out.append(_case("fixed_distance_%d" % s, "distance symbol %d of the fixed code in the data" % s, w, "refuse", BAD_CODE))
    w = Writer()
    syms = []
    for k in range(600):
        syms.append(int(rng.choice([A, A, A, B, B, C_, D_, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a])))
        if k % 5 == 4:
            syms.append((int(rng.choice([3, 4, 258, 227, 250])), int(rng.choice([1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97]))))
    w.dynamic([A] * 200 + syms, COMB_LIT, COMB_DIST, last=1)
    out.append(_case("every_code_length", "every code length 1..15 in both codes: sub-tables of every width, 6 and 9 bits the widest", w))
    return out


# ---- symbols and lane boundaries -----------------------------------------------------------------------------------------------

def _comb_start(w, far=0, last=1):
    """A comb-code section begun, padded with one-bit literals to a 16-bit step of the first tile's grid, and -- far > 0 -- filled
    with 16-bit matches until `far` bytes are made: every lane boundary is a symbol boundary then, and every tile 64 whole lanes.
    -> the bit where the first tile's grid begins"""
    w.dynamic_header(COMB_LIT, COMB_DIST, last=last)
    base = w.pos & ~31
    lit, dist = canonical(COMB_LIT), canonical(COMB_DIST)
    w.symbols([A] * ((16 - (w.pos - base)) % 16), lit, dist)
    while len(w.out) < far or (w.pos - base) % SUB_BITS:
        w.symbols([FILL], lit, dist)
    return base


LONGEST = (227 + 31, 24577 + 8191, 284, 29)             # 15 + 5 + 15 + 13 bits


def _longest_at(name, limit, where, end_after=False):
    """the 48-bit symbol beginning on the bit where(base, pos) names, at or behind pos"""
    w = Writer()
    base = _comb_start(w, 32768)
    lit, dist = canonical(COMB_LIT), canonical(COMB_DIST)
    target = where(base, w.pos)
    while target - w.pos >= 16 + 15:
        w.symbols([FILL], lit, dist)
    w.symbols([A] * (target - w.pos), lit, dist)
    at = w.pos
    w.symbols([LONGEST], lit, dist)
    assert w.pos - at == 48 and at == target
    if not end_after:
        w.symbols([A] * 7 + [FILL] * 40, lit, dist)
    w.symbols([256], lit, dist)
    return _case(name, limit, w, at=at, base=base, n_bits=w.pos)


def symbol_cases():
    rng = np.random.default_rng(103)
    out = []
    out.append(_longest_at("longest_symbol_lane_end", "the 48-bit symbol begins on the last bit of a lane's SUB_BITS bits",
                           lambda base, pos: base + ((pos - base) // TILE_BITS + 1) * TILE_BITS + 21 * SUB_BITS - 1))
    out.append(_longest_at("longest_symbol_tile_end", "the 48-bit symbol begins on the last bit of lane 63: it ends in TILE_PAD",
                           lambda base, pos: base + ((pos - base) // TILE_BITS + 2) * TILE_BITS - 1))
    c = _longest_at("longest_symbol_data_end", "the 48-bit symbol and the 3 bits of the end-of-block code are the block's last bits: the reads go past the data, into the image's padding",
                    lambda base, pos: pos + 40, end_after=True)
    out.append(c)
    out.append(_longest_at("longest_symbol_bit31", "the 48-bit symbol begins on bit 31 of a word", lambda base, pos: (pos + 100) | 31))
    # the second literal of a turn
    lit, dist = canonical(COMB_LIT), canonical(COMB_DIST)
    for name, second, limit in (("root_literal", [D_], "a literal of the root table's longest code: taken"), ("sub_table_literal", [C_], "a literal of a sub-table: not taken, decoded by the next turn"),
                                ("end_of_block", [], "the end-of-block code"), ("length_code", [(3, 1)], "a length code")):
        w = Writer()
        w.dynamic([A, B] * 10 + [A] + second + ([B, A, A] + second) * 3, COMB_LIT, COMB_DIST, last=1)
        out.append(_case("lit2_then_" + name, "a 1-bit literal and behind it " + limit, w))
    for past in (0, 1):
        # fifteen matches and fourteen 1-bit literals, two to a turn: the next turn begins two bits before the lane's end, its first
        # literal ends one bit before it, its second -- 1 or 2 bits -- exactly on the end or one bit past it
        w = Writer()
        base = _comb_start(w)
        w.symbols([FILL] * 15 + [A] * 14, lit, dist)
        at = w.pos
        w.symbols([A, B if past else A] + [A] * 30 + [FILL, 256], lit, dist)
        out.append(_case("lit2_ends_%s_stop" % ("past" if past else "on"), "the second literal of a turn ends %s" %
                         ("one bit past the lane's end" if past else "exactly on the lane's end"), w, at=at, base=base))
    # literal runs inside one lane: matches in front (whole 16-bit steps from the lane's first bit) and behind.  257 and more cannot be:
    # a lane's symbols BEGIN in its SUB_BITS bits, and the shortest code has one.
    for n in (127, 128, 129, 255, 256):
        for shifted in (False, True):
            # shifted: a sub-table literal second -- the turn before it takes one literal alone, so the run's even literals are the
            # FIRST of their turns (else, after a match, they are the second: the 128th literal of a run is then a turn's second)
            head = [A, C_] if shifted else []
            bits = n + (9 if shifted else 0)
            if bits > SUB_BITS:
                continue
            w = Writer()
            base = _comb_start(w)
            w.symbols([FILL] * ((SUB_BITS - bits) // 16), lit, dist)
            at = w.pos
            w.symbols(head + [A] * (n - len(head)), lit, dist)
            end = w.pos
            w.symbols([FILL] + [A] * 5 + [256], lit, dist)
            out.append(_case("run_of_%d%s" % (n, "_shifted" if shifted else ""), "a run of exactly %d literals inside one lane%s%s" %
                             (n, ", the first of each turn the even ones" if shifted else "", ", ending on the lane's last bit" if (end - base) % SUB_BITS == 0 else ""),
                             w, run=n, at=at, end=end, base=base))
    w = Writer()
    w.fixed(_lits(rng, 300) + [(258, 300), (258, 7, 284), (3, 1), (258, 1), (258, 1, 284)], last=1)
    out.append(_case("length_258_both_spellings", "length 258 from symbol 285, and from symbol 284 with extra bits 31; length 258 at distance 1", w))
    w = Writer()
    w.fixed(_lits(rng, 251) + [(258, 251)] * 126 + _lits(rng, 9))
    n = 32768 - len(w.out)
    w.fixed(_lits(rng, n) + [(3, 32768), 5, (3, 32768), (258, 32768)], last=1)
    out.append(_case("length_3_distance_32768", "length 3 at distance 32768, the farthest there is", w))
    # sections that change in the middle of a word
    for phase in (1, 17, 31):
        # (literals of 8 bits and of 9 walk the end of the first section to the bit wanted: 3 + 8 k + 9 j + 7)
        k, j = [(k, j) for j in range(32) for k in range(4, 8) if (10 + 8 * k + 9 * j) % 32 == phase][0]
        w = Writer()
        w.fixed(_lits(rng, k, 144) + [200] * j)
        at = w.pos
        w.dynamic([A, B, A, (3, 1), C_] * 20, COMB_LIT, COMB_DIST)
        w.fixed([1, 2, 3, (6, 2)], last=1)
        out.append(_case("section_at_bit_%d" % phase, "a section whose first symbol's header begins where pos & 31 = %d" % phase, w, at=at, phase=phase))
    w = Writer()
    for k in range(20):
        if k % 3 == 0:
            w.fixed(_lits(rng, 30) + [(20, 9)])
        elif k % 3 == 1:
            w.stored(bytes(_lits(rng, 1 + k)))
            w.stored(b"")
        else:
            w.dynamic([A, B, C_, (3, 2), D_] * 9, COMB_LIT, COMB_DIST)
    w.stored(b"", last=1)
    out.append(_case("twenty_sections", "twenty sections of alternating kinds in one block, stored sections of length 0 between Huffman ones", w))
    # tiles with more tokens than the token room of a tile
    for name, bits, cap_over, cap_under in (("tokcap", 3, TOKCAP, None), ("tokcap_small", 4, TOKCAP_SMALL, TOKCAP)):
        n_sym = 1 << bits
        lit = [0] * 257
        for s in range(n_sym - 1):
            lit[s] = bits
        lit[256] = bits
        w = Writer()
        w.dynamic(_lits(rng, 3 * TILE_BITS // bits, n_sym - 1), lit, [0], last=1)
        per_tile = (SUB_BITS // bits + 1) * 64
        assert per_tile > cap_over and (cap_under is None or per_tile <= cap_under)
        out.append(_case("tile_over_" + name, "literals of %d bits: a whole tile's tokens are %d bytes, more than %s%s" %
                         (bits, per_tile, name.upper(), "" if cap_under is None else " and no more than TOKCAP"), w, per_tile=per_tile))
    # ... and with codes of one bit, where every bit is a symbol boundary and every lane's guess is right: no lane's tokens are written
    # twice, the places do not fit the room, and the tile is cut where its tokens end
    for name, lane, cap_over, cap_under in (("tokcap", [A] * SUB_BITS, TOKCAP, None), ("tokcap_small", [FILL] * (SUB_BITS // 16 - 2) + [A] * 32, TOKCAP_SMALL, TOKCAP)):
        w = Writer()
        _comb_start(w)
        w.symbols(lane * (3 * 64) + [256], canonical(COMB_LIT), canonical(COMB_DIST))
        per_tile = sum(1 if isinstance(s, int) else 3 for s in lane) * 64 + 64 * (2 if name == "tokcap" else 1)
        assert per_tile > cap_over and (cap_under is None or per_tile <= cap_under)
        out.append(_case("tile_over_%s_right_guesses" % name, "1-bit literals, every lane's guess right: a whole tile's tokens are %d bytes, more than %s%s" %
                         (per_tile, name.upper(), "" if cap_under is None else " and no more than TOKCAP"), w, per_tile=per_tile))
    w = Writer()
    w.stored(bytes(_lits(rng, 65531)), last=1)
    out.append(_case("in_len_65536", "in_len = 65536: one stored section of 65531 bytes", w))
    w = Writer()
    w.fixed(_lits(rng, 251) + [(258, 251)] * 253 + [(11, 251)], last=1)
    assert len(w.out) == 65536
    out.append(_case("out_len_65536", "out_len = 65536", w))
    w = Writer()
    w.fixed(_lits(rng, 500) + [(100, 300), 7], last=1)
    comp = w.done()
    out.append(_case("one_byte_more", "a stream that makes one byte more than out_len", comp, "refuse", OVERRUN, data=bytes(w.out[:-1]), stream_is_legal=True))
    out.append(_case("one_byte_fewer", "a stream that makes one byte fewer than out_len", comp, "refuse", SHORT, data=bytes(w.out) + b"\0", stream_is_legal=True))
    # a lane whose guessed start sees something else altogether: three 9-bit literals put every lane's first bit two bits into the
    # code of literal 16 (01000000), and with literal 0 (00110000) behind it the guess reads seven zeros, the end-of-block code: the
    # lane's place is sized for no tokens at all, its true tokens (32 literals) do not fit it and are written again
    w = Writer()
    w.fixed([200, 200, 200] + [16, 0] * 600, last=1)
    out.append(_case("guess_sees_end_of_block", "every lane's guessed decode ends at once: places too small for the true tokens (misfit, written again)", w))
    return out


# ---- distances against the block's start ---------------------------------------------------------------------------------------

def distance_cases():
    rng = np.random.default_rng(104)
    out = []
    for over in (0, 1):
        kind, code = ("refuse", BAD_DISTANCE) if over else ("legal", None)
        what = "one more than the bytes made so far" if over else "equal to the bytes made so far"
        w = Writer()
        w.fixed(_lits(rng, 9) + [(20, 9 + over), 1, 2], last=1)
        out.append(_case("distance_%s_lane0" % ("over" if over else "full"), "lane 0 of the first tile: a distance " + what, w, kind, code))
        w = Writer()
        w.fixed(_lits(rng, 200) + [(20, 200 + over), 1, 2], last=1)
        out.append(_case("distance_%s_later_lane" % ("over" if over else "full"), "a later lane of the first tile: a distance " + what, w, kind, code, lane_bit=200 * 8))
        w = Writer()
        w.fixed(_lits(rng, 2300, 144) + [(20, 2300 + over), 1, 2], last=1)
        out.append(_case("distance_%s_second_tile" % ("over" if over else "full"), "the second tile: a distance " + what, w, kind, code, lane_bit=2300 * 8))
        w = Writer()
        w.fixed(_lits(rng, 100))
        w.stored(bytes(_lits(rng, 33)))
        w.fixed([0x41] * 50 + [(9, 183 + over), 0x42], last=1)
        out.append(_case("distance_%s_second_section" % ("over" if over else "full"), "a later section: a distance " + what, w, kind, code))
    return out


# ---- the copying kernel --------------------------------------------------------------------------------------------------------

SWEEP_DIST = sorted(set(list(range(1, 65)) + [RING - 17, RING - 16, RING - 15, 255, 256, 257, 258, 32767, 32768]))
SWEEP_LEN = [3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 257, 258]


def sweep_block(dist, length, phase, seed=0):
    """random bytes up to an output position with (position & 15) = phase and at least `dist`, the match, a literal, the match again
    (far prefixes are themselves matches of period 251, then a run of literals: the stream stays small)"""
    rng = np.random.default_rng((dist << 16) ^ (length << 4) ^ phase ^ (seed << 40))
    want = dist + (phase - dist) % 16
    w = Writer()
    if want <= 300:
        syms = _lits(rng, want)
    else:
        syms, made = _lits(rng, 251), 251
        while want - made > 40:
            n = min(258, want - made - 20)
            syms.append((n, 251))
            made += n
        syms += _lits(rng, want - made)
    w.fixed(syms + [(length, dist), int(rng.integers(0, 256)), (length, dist)], last=1)
    return Case("sweep_d%d_l%d_p%d" % (dist, length, phase), "copy_block: distance %d, length %d, output phase %d" % (dist, length, phase), "legal",
                w.done(), bytes(w.out), None, {"dist": dist, "length": length, "phase": phase})


def sweep(full):
    """full: every distance x length x phase.  Otherwise a covering subset: every distance, length and phase at least once, and every
    (distance, length) pair for the distances below 8, at 8 and around RING - 16, the phases rotating."""
    return [sweep_block(*p) for p in sweep_params(full)]


def sweep_params(full):
    if full:
        return [(d, n, p) for d in SWEEP_DIST for n in SWEEP_LEN for p in range(16)]
    picks = [(d, SWEEP_LEN[k % len(SWEEP_LEN)], (5 * k) % 16) for k, d in enumerate(SWEEP_DIST)]
    k = 0
    for d in list(range(1, 9)) + [RING - 17, RING - 16, RING - 15]:
        for n in SWEEP_LEN:
            picks.append((d, n, (7 * k) % 16))
            k += 1
    return sorted(set(picks))


def copy_cases():
    rng = np.random.default_rng(105)
    out = []
    w = Writer()
    w.fixed(_lits(rng, 400) + [(40, 100), (40, 200), (258, 300), (258, RING - 15), (17, 400), (16, 399), (33, 398), 1, (100, 64), (3, 70), (3, 71)], last=1)
    out.append(_case("far_behind_far", "far matches directly behind far matches, long ones among them: the next piece asked for a turn ahead", w))
    for run in (1, 17, 40):
        syms = _lits(rng, 200)
        for d in range(RING - 15, RING + 49):
            syms += _lits(rng, run) + [(20, d)]
        w = Writer()
        w.fixed(syms, last=1)
        out.append(_case("far_behind_run_of_%d" % run, "far matches behind literal runs of %d at 64 consecutive distances: the source's first piece ends on, below "
                         "and above what is in memory when the second reader gets there" % run, w))
    for seed in range(4):
        syms = _lits(rng, 30)
        for k in range(700):
            syms += _lits(rng, int(rng.integers(0, 6)))
            if k % 2 or rng.random() < 0.5:
                syms.append((int(rng.integers(3, 24)), int(rng.integers(1, 25))))
        w = Writer()
        w.fixed(syms, last=1)
        out.append(_case("token_offsets_%d" % seed, "short literal runs and matches by the hundred: tokens on every offset of the 64-byte beat and across the FIFO's wrap", w))
    w = Writer()
    w.fixed(_lits(rng, 20) + [(40, 13)], last=1)
    out.append(_case("match_ends_block", "a match that ends on the block's last byte", w))
    w = Writer()
    w.fixed([0x5a], last=1)
    out.append(_case("one_byte", "a block of one byte", w))
    for tail in range(1, 16):
        w = Writer()
        w.fixed(_lits(rng, 10) + ([(6 + tail, 10)] if tail % 2 else [(6, 3)] + _lits(rng, tail)), last=1)
        assert len(w.out) % 16 == tail
        out.append(_case("tail_of_%d" % tail, "a block whose last 16-byte piece holds %d bytes" % tail, w))
    return out


_CACHE = {}


def named_cases():
    if "named" not in _CACHE:
        _CACHE["named"] = header_cases() + table_cases() + symbol_cases() + distance_cases() + copy_cases()
        names = [c.name for c in _CACHE["named"]]
        assert len(set(names)) == len(names)
    return _CACHE["named"]


def image_of(cases):
    """-> (image bytes with SPL_Z_IMAGE_PAD zeros behind, spl_zblock rows, each block's offset in the output, the output's length)"""
    image = bytearray()
    blocks = np.zeros((len(cases), 4), np.uint64)   # spl_zblock: in, out, (in_len | out_len << 32), (crc | pad << 32)
    starts, at = [], 0
    for k, c in enumerate(cases):
        blocks[k] = (len(image), at, len(c.comp) | (len(c.data) << 32), zlib.crc32(c.data) & 0xffffffff)
        image += c.comp
        starts.append(at)
        at += len(c.data)
    image += bytes(SPL_Z_IMAGE_PAD)
    return bytes(image), blocks, starts, at


def check(case, status, got, reference=None):
    """the policy of this module's docstring for one block: status word and the block's stretch of the output"""
    if case.kind == "legal":
        assert status == OK, (case.name, case.limit, int(status))
        assert got == case.data, (case.name, case.limit)
    elif case.kind == "refuse":
        assert status != OK, (case.name, case.limit)
        if case.code is not None:
            assert status == case.code, (case.name, case.limit, int(status), case.code)
    else:
        assert status != OK or got == (reference if reference is not None else inflate(case.comp)), (case.name, case.limit, int(status))


def refusals_between_legal(cases):
    """the same cases, every one that is not legal between two legal ones"""
    legal, other = [c for c in cases if c.kind == "legal"], [c for c in cases if c.kind != "legal"]
    assert len(legal) > len(other)
    out = []
    for k, c in enumerate(other):
        out += [legal[k], c]
    return out + legal[len(other):]


# ---- whole payloads, parsed perversely (the BGZF blocks of test_gpu_inflate_limits.py's files) -----------------------------------

def parse(data, mode):
    """LZ77 over `data` -> symbols.  len3_farthest: matches of length 3 only, each at the farthest earlier occurrence in reach;
    longest_far: the longest match among the oldest occurrences at distance >= RING - 15, wherever there is one; greedy: the longest
    among the newest occurrences."""
    from bisect import bisect_left
    n, i, added, syms, seen = len(data), 0, 0, [], {}
    while i < n:
        while added < i:
            if added + 3 <= n:
                seen.setdefault(data[added:added + 3], []).append(added)
            added += 1
        best = None
        cand = seen.get(data[i:i + 3]) if i + 3 <= n else None
        if cand:
            k = bisect_left(cand, i - 32768)
            if mode == "len3_farthest":
                if k < len(cand):
                    best = (3, i - cand[k])
            else:
                pool = [p for p in cand[k:k + 8] if i - p >= RING - 15] if mode == "longest_far" else [p for p in cand[-8:] if p >= i - 32768]
                for p in pool:
                    length = 3
                    while length < 258 and i + length < n and data[p + length] == data[i + length]:
                        length += 1
                    if best is None or length > best[0]:
                        best = (length, i - p)
        if best:
            syms.append(best)
            i += best[0]
        else:
            syms.append(data[i])
            i += 1
    return syms


def skewed_lens(freq, size):
    """A complete code, as lopsided as 15 bits allow: the most frequent symbols get 1, 2, 3, .. bits, the rest share what is left"""
    order = sorted(freq, key=lambda s: (-freq[s], s))
    lens, n = [0] * size, len(order)
    if n == 1:
        lens[order[0]] = 1
        return lens
    m = min(n - 2, 13)
    while m + max(flat_lens(n - m)) > 15:
        m -= 1
    rest = flat_lens(n - m)
    for k, s in enumerate(order):
        lens[s] = k + 1 if k < m else m + rest[k - m]
    return lens


def rle_of(lens):
    """a run-length spelling: runs of zeros by 17 and 18, runs of another length by 16, the rest plainly"""
    out, k = [], 0
    while k < len(lens):
        j = k
        while j < len(lens) and lens[j] == lens[k]:
            j += 1
        run = j - k
        if lens[k] == 0 and run >= 3:
            take = min(run, 138)
            out.append((18 if take >= 11 else 17, take))
        elif lens[k] != 0 and run >= 4:
            take = min(run - 1, 6)
            out += [lens[k], (16, take)]
            take += 1
        else:
            take = 1
            out.append(lens[k])
        k += take
    return out


def _section_codes(syms):
    fl, fd = {256: 1}, {}
    for s in syms:
        if isinstance(s, int):
            fl[s] = fl.get(s, 0) + 1
        else:
            fl[length_symbol(s[0])] = fl.get(length_symbol(s[0]), 0) + 1
            fd[distance_symbol(s[1])] = fd.get(distance_symbol(s[1]), 0) + 1
    return skewed_lens(fl, 286), (skewed_lens(fd, 30) if fd else [0] * 30)


PERVERSE = ("len3_farthest", "longest_far", "dynamic_every_200", "alternating")


def perverse_deflate(payload, variant):
    """`payload` as one DEFLATE stream, written the way `variant` names"""
    w = Writer()
    if variant == "len3_farthest":
        w.fixed(parse(payload, "len3_farthest"), last=1)
    elif variant == "longest_far":
        syms = parse(payload, "longest_far")
        lit, dist = _section_codes(syms)
        w.dynamic(syms, lit, dist, last=1, rle=rle_of(lit + dist))
    else:
        syms = parse(payload, "greedy")
        step = 200 if variant == "dynamic_every_200" else 300
        chunks = [syms[k:k + step] for k in range(0, len(syms), step)]
        for k, chunk in enumerate(chunks):
            last = int(k == len(chunks) - 1)
            kind = 2 if variant == "dynamic_every_200" else k % 3
            if kind == 0:
                at = len(w.out)
                w.stored(payload[at:at + sum(1 if isinstance(s, int) else s[0] for s in chunk)], last=last)
            elif kind == 1:
                w.fixed(chunk, last=last)
            else:
                lit, dist = _section_codes(chunk)
                w.dynamic(chunk, lit, dist, last=last, rle=rle_of(lit + dist))
    assert bytes(w.out) == bytes(payload)
    return w.done()
