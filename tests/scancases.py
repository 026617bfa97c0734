"""Hand-built BAM record streams for the device's record scan, extraction and bounds kernels (spl_inflate.hip), with a plain
restatement of what they must leave.  Shared by test_scancases_host.py (CPU: the cases are what they say, the restatement agrees
with the host decoder) and test_gpu_bam_scan_limits.py (the kernels against the restatement, field for field).

A case is a stream (BAM header bytes + raw records, each built field by field from the SAM specification, section 4.2, so that
illegal ones can be built too), a table of blocks laid over it as a tiling the case chooses, and the scan's other arguments.
`reference_scan` says per block what `struct spl_bscan` (spl_inflate.h) and the launchers' comments promise; `reference_extract`
says what the extraction leaves for the placed records.  Both are walks over the bytes in Python, written from the format and
the header's words.  The numbers of the plausibility rule are read from the source, so the cases follow a retune.

Where the header leaves a field open the restatement fixes it here, once:
  * a block flagged SPL_BS_NO_START has `start` = `reached` = the first offset the search did not test (the block's first byte
    where it tested none): the search's own account of how far it came;
  * a block of BAM header bytes only has `start` = `reached` = its end, and no record.
Nothing here touches the GPU."""
import os
import re
import struct

import numpy as np

import xscases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spliser_amd", "csrc")

ZBLOCK = np.dtype([("in", "<u8"), ("out", "<u8"), ("in_len", "<u4"), ("out_len", "<u4"), ("crc", "<u4"), ("pad", "<u4")])
BSCAN = np.dtype([("start", "<u8"), ("reached", "<u8"), ("n_all", "<u4"), ("n_placed", "<u4"), ("n_ops", "<u4"), ("flags", "<u4"),
                  ("tid_first", "<i4"), ("tid_last", "<i4"), ("n_foreign", "<u4"), ("n_foreign_hi", "<u4"), ("n_drop_flags", "<u4"),
                  ("n_drop_mapq", "<u4")])
assert ZBLOCK.itemsize == 32 and BSCAN.itemsize == 56

M, I, D, N, S, H, P, EQ, X = 0, 1, 2, 3, 4, 5, 6, 7, 8


def _source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _one(pattern, text, what):
    found = set(re.findall(pattern, text))
    assert len(found) == 1, (what, pattern, found)
    return found.pop()


_HIP, _HDR = _source("spl_inflate.hip"), _source("spl_inflate.h")
REC_CAP = int(_one(r"#define\s+SPL_BS_REC_CAP\s+(\d+)u", _HDR, "places per block"))
CORRUPT, NEEDS_HOST, UNSORTED, NO_START, INCOMPLETE = (int(_one(r"#define\s+SPL_BS_%s\s+(\d+)u" % n, _HDR, n))
                                                       for n in ("CORRUPT", "NEEDS_HOST", "UNSORTED", "NO_START", "INCOMPLETE"))
REACH = 1 << int(_one(r"u0 \+ \(1ull << (\d+)\)", _HIP, "the reach of the guess"))
CHAIN = int(_one(r"k < (\d+) && ok", _HIP, "successors that must chain"))
HEAD_BYTES = int(_one(r"at \+ (\d+) <= limit", _HIP, "bytes a candidate needs in front of the limit"))
assert HEAD_BYTES == int(_one(r"q \+ (\d+) <= stream_len", _HIP, "bytes a successor needs")) == int(_one(r"end - c < (\d+)\)", _HIP, "bytes a record header needs"))
_m = re.search(r"bs < (\d+)u \|\| bs > \(1u << (\d+)\)", _HIP)
PLAUSIBLE_MIN_BS, PLAUSIBLE_MAX_BS = int(_m.group(1)), 1 << int(_m.group(2))
WALK_MIN_BS = int(_one(r"if \(bs < (\d+)u\) \{ out\.flags", _HIP, "the smallest block_size the walk accepts"))
_m = re.search(r"name\[i\] < (\d+) \|\| name\[i\] > (\d+)", _HIP)
NAME_LO, NAME_HI = int(_m.group(1)), int(_m.group(2))
PAD = 1024          # bytes the GPU test allocates behind a stream (test_scancases_host.py shows it is enough)


# ---- builders --------------------------------------------------------------------------------------------------------------
def op(length, code):
    return (length << 4) | code


def record(tid=0, pos=0, name=b"r\x00", mapq=60, bin_=4681, flag=0, cigar=(), seq=b"", qual=b"", aux=b"", next_tid=-1, next_pos=-1, tlen=0,
           l_name=None, n_cigar=None, l_seq=None, block_size=None):
    """One record's bytes (SAM specification 4.2): every field can be overridden, the counts and the size word apart from the bytes
    they count.  `seq` is the packed bases ((l_seq + 1) / 2 bytes), `qual` l_seq bytes."""
    l_seq = len(qual) if l_seq is None else l_seq
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name) if l_name is None else l_name, mapq, bin_, len(cigar) if n_cigar is None else n_cigar,
                       flag, l_seq, next_tid, next_pos, tlen)
    body += name + struct.pack("<%dI" % len(cigar), *cigar) + seq + qual + aux
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def bam_header(n_ref, text_len=0):
    text = b"@HD\tVN:1.6\tSO:coordinate\n"
    text += b"@" * max(0, text_len - len(text))
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", n_ref)
    for k in range(n_ref):
        nm = b"c%d\x00" % k
        out += struct.pack("<i", len(nm)) + nm + struct.pack("<i", 0x7FFFFFFF)
    return out


def ref_names(n_ref):
    return ["c%d" % k for k in range(n_ref)]


class Case(object):
    """name; data = the whole buffer's meaningful bytes (the stream, and for a window what lies behind stream_len); header_end;
    offsets = where every TRUE record begins; lens = the blocks' lengths (they tile [0, stream_len)); the scan's arguments."""

    def __init__(self, name, family, header, records, lens=None, n_ref=3, stream_len=None, more=0, tid_lo=0, tid_hi=None, filt=(0, 0, 0), junk=None,
                 tail=b"", notes=None):
        self.name, self.family, self.n_ref = name, family, n_ref
        self.header_end = len(header)
        self.offsets, at = [], len(header)
        for r in records:
            self.offsets.append(at)
            at += len(r)
        self.records = list(records)
        self.data = header + b"".join(records) + tail
        self.stream_len = len(self.data) if stream_len is None else stream_len
        self.more, self.tid_lo, self.tid_hi, self.filt = more, tid_lo, n_ref + 1 if tid_hi is None else tid_hi, filt
        self.junk = junk                      # None: the bytes behind stream_len are the stream's own; else a seed for random ones
        self.lens = None if lens is None else np.asarray(lens, np.int64)
        self.notes = notes or {}

    def with_table(self, suffix, lens, **changes):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.name = self.name + "/" + suffix
        c.lens = np.asarray(lens, np.int64)
        c.notes = dict(self.notes)
        c.__dict__.update(changes)
        assert int(c.lens.sum()) == c.stream_len, (c.name, int(c.lens.sum()), c.stream_len)
        return c

    def blocks(self):
        t = np.zeros(len(self.lens), ZBLOCK)
        t["out_len"] = self.lens
        t["out"] = np.concatenate(([0], np.cumsum(self.lens)[:-1]))
        return t

    def buffer(self):
        """The bytes the GPU test uploads: the stream up to stream_len, what lies behind it, and PAD bytes of 0xEE."""
        body = self.data[:self.stream_len]
        behind = self.data[self.stream_len:]
        if self.junk is not None:
            behind = bytes(np.random.default_rng(self.junk).integers(0, 256, max(len(behind), 64), dtype=np.uint8))
        return body + behind + b"\xee" * PAD

    def payloads(self):
        """The blocks' bytes, for a file with one BGZF block per table entry."""
        ends = np.cumsum(self.lens)
        return [self.data[int(e - n):int(e)] for e, n in zip(ends, self.lens)]


def tile(total, length, first=None):
    """Blocks of `length` over [0, total); `first` = bytes the leading blocks cover exactly (a cut falls there)."""
    lens = []
    for lo, hi in ((0, first or 0), (first or 0, total)):
        n = hi - lo
        lens += [length] * (n // length) + ([n % length] if n % length else [])
    return lens


def with_empty(lens, rng, n, at=()):
    """The tiling with zero-length blocks dropped in: in front, behind, at the block indices `at`, and at n random places."""
    lens = list(lens)
    where = sorted(set(int(x) for x in rng.integers(0, len(lens) + 1, n)) | {0, len(lens)} | set(at), reverse=True)
    for w in where:
        lens.insert(w, 0)
        if rng.random() < 0.3:
            lens.insert(w, 0)
    return lens


# ---- the plain reference ---------------------------------------------------------------------------------------------------
class _Bytes(object):
    """The readable stream [0, stream_len) with the fixed-field half of the plausibility rule worked out for every offset at once
    (numpy: a 1.3 MB stream has 1.3 M candidates), and a note of the farthest byte anybody asked for."""

    def __init__(self, data, stream_len, n_ref):
        self.b = bytes(data[:stream_len])
        self.n = stream_len
        self.n_ref = n_ref
        self.far = 0
        self._fixed = None
        self._plaus = {}

    def u32(self, at):
        self.far = max(self.far, at + 4)
        return struct.unpack_from("<I", self.b, at)[0]

    def i32(self, at):
        self.far = max(self.far, at + 4)
        return struct.unpack_from("<i", self.b, at)[0]

    def fixed_ok(self):
        if self._fixed is None:
            a = np.frombuffer(self.b + b"\x00" * 40, np.uint8).astype(np.int64)
            n = max(self.n - HEAD_BYTES + 1, 0)

            def u32(off):
                return a[off:off + n] | (a[off + 1:off + 1 + n] << 8) | (a[off + 2:off + 2 + n] << 16) | (a[off + 3:off + 3 + n] << 24)

            def i32(off):
                v = u32(off)
                return np.where(v >= 1 << 31, v - (1 << 32), v)
            bs, tid, pos, l_name, n_cig = u32(0), i32(4), i32(8), a[12:12 + n], a[16:16 + n] | (a[17:17 + n] << 8)
            l_seq, ntid, npos = i32(20), i32(24), i32(28)
            ok = (bs >= PLAUSIBLE_MIN_BS) & (bs <= PLAUSIBLE_MAX_BS) & (tid >= -1) & (tid < self.n_ref) & (ntid >= -1) & (ntid < self.n_ref)
            ok &= (pos >= -1) & (npos >= -1) & (l_seq >= 0) & (l_name >= 1)
            ok &= 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq <= bs
            self._fixed = np.flatnonzero(ok)
            self._fixed_set = set(self._fixed.tolist())
        return self._fixed

    def plausible(self, c):
        """-> the record's size with its length word, or 0.  SAM 4.2: block_size covers a fixed part of 32 bytes, a NUL-terminated
        name of printable characters, and CIGAR, SEQ and QUAL of the lengths the fixed part states; reference ids are -1 or a
        reference of the header, positions -1 or more.  Needs 36 bytes; the name is judged where all of it is there."""
        if c in self._plaus:
            return self._plaus[c]
        size = 0
        if self.n - c >= HEAD_BYTES:
            self.fixed_ok()
            self.far = max(self.far, c + HEAD_BYTES)
            if c in self._fixed_set:
                l_name = self.b[c + 12]
                size = 4 + struct.unpack_from("<I", self.b, c)[0]
                if self.n - c >= 36 + l_name:
                    self.far = max(self.far, c + 36 + l_name)
                    name = self.b[c + 36:c + 36 + l_name]
                    if name[-1] != 0 or any(x < NAME_LO or x > NAME_HI for x in name[:-1]):
                        size = 0
        self._plaus[c] = size
        return size

    def chained(self, c):
        size = self.plausible(c)
        if not size:
            return False
        q = c + size
        for _ in range(CHAIN):
            if q + HEAD_BYTES > self.n:          # (near the stream's end the chain is as long as the bytes allow)
                break
            size = self.plausible(q)
            if not size:
                return False
            q += size
        return True

    def guess(self, u0):
        """-> (found, offset): the first chained candidate c >= u0 with c + 36 <= min(u0 + reach, stream_len), or where the search ended."""
        limit = min(u0 + REACH, self.n)
        cands = self.fixed_ok()
        k = int(np.searchsorted(cands, u0))
        while k < len(cands) and cands[k] + HEAD_BYTES <= limit:
            c = int(cands[k])
            if self.chained(c):
                self.far = max(self.far, c + HEAD_BYTES)
                return True, c
            k += 1
        ended = max(u0, limit - HEAD_BYTES + 1)
        if limit - HEAD_BYTES >= u0:
            self.far = max(self.far, limit)
        return False, ended


def verdict(filt, flag, mapq):
    """0 kept, 1 dropped by its flags, 2 dropped by its MAPQ (spl_bam.h: flags are judged first)."""
    min_mapq, require, exclude = filt
    if flag & exclude or (flag & require) != require:
        return 1
    return 0 if mapq >= min_mapq else 2


def reference_scan(stream, stream_len, header_end, n_ref, tid_lo, tid_hi, blocks, more, filt):
    """-> (BSCAN array, the places of each block's placed records, the farthest byte offset read + 1)."""
    by = _Bytes(stream, stream_len, n_ref)
    out = np.zeros(len(blocks), BSCAN)
    places = []
    for b in range(len(blocks)):
        u0 = int(blocks["out"][b])
        u1 = u0 + int(blocks["out_len"][b])
        s = dict(n_all=0, n_placed=0, n_ops=0, flags=0, tid_first=-1, tid_last=-1, n_foreign=0, n_foreign_hi=0, n_drop_flags=0, n_drop_mapq=0)
        mine = []
        places.append(mine)
        empty_at_header_end = u0 == u1 == header_end
        if u1 <= header_end and not empty_at_header_end:      # BAM header bytes only
            s["start"] = s["reached"] = u1
            for k, v in s.items():
                out[k][b] = v
            continue
        if u0 <= header_end:
            at = header_end                                   # the first record of the file: known
        else:
            found, at = by.guess(u0)
            if not found:
                if min(u0 + REACH, stream_len) == stream_len:
                    if more:
                        s["flags"] |= INCOMPLETE | NO_START   # whatever starts here ends beyond the window
                    else:
                        at = stream_len                       # the tail of the file's last record
                else:
                    s["flags"] |= NO_START
        s["start"] = at
        last_tid = -1
        while at < u1 and not s["flags"] & (CORRUPT | NO_START | INCOMPLETE):
            short = INCOMPLETE if more else CORRUPT
            if stream_len - at < 4:
                s["flags"] |= short
                break
            bs = by.u32(at)
            if bs < WALK_MIN_BS:
                s["flags"] |= CORRUPT
                break
            if stream_len - at < 4 + bs:
                s["flags"] |= short
                break
            tid, pos0 = by.i32(at + 4), by.i32(at + 8)
            l_name, mapq = by.b[at + 12], by.b[at + 13]
            n_cig, flag = struct.unpack_from("<HH", by.b, at + 16)
            l_seq = by.u32(at + 20)
            need = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
            if need > bs:
                s["flags"] |= CORRUPT
                break
            tid_eff = tid if 0 <= tid < n_ref else n_ref
            if tid_eff < last_tid:
                s["flags"] |= UNSORTED
            last_tid = tid_eff
            if not tid_lo <= tid_eff < tid_hi:
                s["n_foreign"] += 1
                s["n_foreign_hi"] += tid_eff >= tid_hi
                at += 4 + bs
                continue
            s["n_all"] += 1
            placed = 0 <= tid < n_ref and pos0 >= 0
            v = verdict(filt, flag, mapq) if placed else 0
            if v == 1:
                s["n_drop_flags"] += 1
            elif v == 2:
                s["n_drop_mapq"] += 1
            elif placed:
                if n_cig and bs > need:
                    op0 = by.u32(at + 36 + l_name)
                    if op0 & 15 == S and op0 >> 4 == l_seq:
                        s["flags"] |= NEEDS_HOST
                if s["tid_first"] < 0:
                    s["tid_first"] = tid
                s["tid_last"] = tid
                mine.append(at - u0)
                s["n_placed"] += 1
                s["n_ops"] += n_cig
            at += 4 + bs
        s["reached"] = at
        for k, v in s.items():
            out[k][b] = v
    return out, places, by.far


def reference_extract(stream, offsets, n_ref, tid_lo, tid_hi, filt, cig_off0=0):
    """What the extraction leaves for the records at `offsets` (true boundaries, in stream order): dict of pos, flag, tid, cig_off
    (one more than records, beginning with cig_off0), cigar, xs, and ref_max_end per reference as Python ints."""
    pos, flag, tids, cig_off, cigar, xs = [], [], [], [cig_off0], [], []
    max_end = [0] * max(n_ref, 1)
    for at in offsets:
        bs, tid, pos0, l_name, mapq, _bin, n_cig, fl, l_seq = struct.unpack_from("<IiiBBHHHI", stream, at)
        if not (0 <= tid < n_ref and pos0 >= 0 and tid_lo <= tid < tid_hi) or verdict(filt, fl, mapq):
            continue
        ops = struct.unpack_from("<%dI" % n_cig, stream, at + 36 + l_name)
        ref_len = sum(o >> 4 for o in ops if o & 15 in (M, D, N, EQ, X))
        aux = stream[at + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq:at + 4 + bs]
        pos.append(pos0 + 1)
        flag.append(fl)
        tids.append(tid)
        cigar.extend(ops)
        cig_off.append(cig_off0 + len(cigar))
        xs.append(xscases.py_walk(aux) if any(o & 15 == N for o in ops) else 0)
        max_end[tid] = max(max_end[tid], pos0 + 1 + max(ref_len, 1) - 1)
    return dict(pos=np.asarray(pos, np.int32), flag=np.asarray(flag, np.uint16), tid=np.asarray(tids, np.int32), cig_off=np.asarray(cig_off, np.uint32),
                cigar=np.asarray(cigar, np.uint32), xs=np.asarray(xs, np.uint8), ref_max_end=max_end)


_REFERENCE = {}


def reference(case):
    """(scan, places, far) of a case, computed once."""
    if case.name not in _REFERENCE:
        buf = case.buffer()
        _REFERENCE[case.name] = reference_scan(buf, case.stream_len, case.header_end, case.n_ref, case.tid_lo, case.tid_hi, case.blocks(), case.more, case.filt)
    return _REFERENCE[case.name]


def extractable(scan):
    """What records_done (spl_capi.cpp) lets through to the extraction: no block CORRUPT, NO_START or INCOMPLETE."""
    return not np.any(scan["flags"] & (CORRUPT | NO_START | INCOMPLETE))


def decline_reason(case, scan):
    """'' if the device decoder must take a file of these blocks, else what it must say (records_done, one window, tid window
    (0, n_ref + 1)): the first complaint in block order."""
    blocks = case.blocks()
    expect, last_tid = case.header_end, -1
    for b in range(len(scan)):
        sc = scan[b]
        if int(blocks["out"][b]) + int(blocks["out_len"][b]) <= case.header_end and b + 1 < len(scan):     # BAM header only
            continue
        f = int(sc["flags"])
        if f & CORRUPT:
            return "a record contradicts itself"
        if f & NO_START:
            return "no record boundary found near a block"
        if f & NEEDS_HOST:
            return "a CIGAR parked in a CG tag"
        if f & UNSORTED:
            return "not sorted by reference"
        if int(sc["start"]) != expect:
            return "a guessed record boundary did not hold"
        if sc["n_placed"] and sc["tid_first"] < last_tid:
            return "not sorted by reference"
        if sc["n_placed"]:
            last_tid = int(sc["tid_last"])
        expect = int(sc["reached"])
    return "" if expect == case.stream_len else "the file ends inside a record"


def true_start(case, u0):
    """The first true record boundary at or after u0 (the stream's end counts as one)."""
    for o in case.offsets:
        if o >= u0:
            return o
    return len(case.data) - len(case.notes.get("tail", b""))


# ---- the case families -----------------------------------------------------------------------------------------------------
def _name(rng, n):
    """n bytes of name with the NUL (n = 1: the empty name)."""
    return bytes(rng.integers(NAME_LO, NAME_HI + 1, n - 1, dtype=np.uint8)) + b"\x00"


def _noise(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def _short_records(rng, n, n_ref=3, aux=None, flags=(0, 16, 99, 147, 83, 163, 256, 1024), mapqs=(60,)):
    """n short records sorted by reference, mixed: placed, pos -1, no CIGAR, unmapped-but-placed, l_seq odd and even, names of 1
    and 255 bytes; SEQ and QUAL are random bytes.  The tail is without a reference."""
    recs = []
    pos = 0
    for k in range(n):
        tid = min(k * (n_ref + 1) // n, n_ref)
        tid = -1 if tid == n_ref else tid
        kind = int(rng.integers(0, 10))
        pos += int(rng.integers(0, 300))
        l_name = 1 if k % 11 == 3 else 255 if k % 29 == 7 else int(rng.integers(2, 30))
        l_seq = int(rng.integers(0, 40))
        n_cig = 0 if kind == 0 else int(rng.choice([1, 1, 2, 3, 5]))
        cig = [op(int(rng.integers(1, 90)), N if j % 2 else int(rng.choice([M, M, EQ, X, I, S]))) for j in range(n_cig)]
        fl = int(rng.choice(flags)) | (4 if kind == 1 else 0)
        if k % 17 == 4:                        # the smallest record there is with a name: 37 bytes
            l_name, l_seq, n_cig, cig = 1, 0, 0, []
        room = 150 - 36 - l_name - 4 * n_cig
        l_seq = max(0, min(l_seq, (room - 1) * 2 // 3)) if l_name < 100 else l_seq
        a = b"" if aux is None else aux(rng)
        recs.append(record(tid=tid, pos=-1 if (kind == 2 or tid < 0) else pos, name=_name(rng, l_name), mapq=int(rng.choice(mapqs)), flag=fl, cigar=cig,
                           seq=_noise(rng, (l_seq + 1) // 2), qual=_noise(rng, l_seq), aux=a, next_tid=tid if kind == 3 else -1,
                           next_pos=pos + 200 if kind == 3 else -1))
    return recs


LENGTHS = (1, 2, 3, 4, 7, 36, 37, 61, 4096, 65536)


def family1():
    """Every cut phase: each tiling with the header's end inside a block, at a block's end and at a zero-length block, and
    again with zero-length blocks dropped in."""
    rng = np.random.default_rng(101)
    recs = _short_records(rng, 60)
    out = []
    for L in LENGTHS:
        header = bam_header(3, text_len=64 if L != 7 and L != 4 else 66)
        base = Case("cuts", 1, header, recs)
        H, total = base.header_end, base.stream_len
        inside = tile(total, L)
        at_end = tile(total, L, first=H)
        n_head = len(tile(H, L))
        tables = [("inside", inside), ("at_end", at_end), ("at_empty", at_end[:n_head] + [0] + at_end[n_head:])]
        for how, lens in tables:
            out.append(base.with_table("L%d/%s" % (L, how), lens, notes=dict(header=how, L=L)))
            out.append(base.with_table("L%d/%s/empties" % (L, how), with_empty(lens, rng, 6, at=(n_head,) if how != "inside" else ()), notes=dict(header=how, L=L)))
    return out


def family2():
    """Records larger than blocks, 64 KiB blocks: a 200 KB record, and one of more than 1 MiB + 128 KB whose end lies exactly the
    guess's reach from a block's first byte -- in three tilings, shifted by a byte either way."""
    rng = np.random.default_rng(202)
    header = bam_header(3, text_len=100)
    small = _short_records(rng, 24, n_ref=1)
    a, b, c = [r for r in small[:18]], small[18:21], small[21:]
    a = [r for r in a if struct.unpack_from("<i", r, 4)[0] == 0]
    big200 = record(tid=0, pos=90000, name=b"big200\x00", cigar=[op(134000, M)], seq=b"\x11" * 67000, qual=b"\x1e" * 134000)
    out = []
    # the 200 KB record alone: every block finds a start within reach
    c200 = Case("big/200K", 2, header, a[:6] + [big200] + a[6:] + c)
    out.append(c200.with_table("64K", tile(c200.stream_len, 65536), notes=dict(big=len(big200))))
    # the large one: sized so that, under the tiling, block B's first byte + reach - 36 is exactly where the record behind it begins
    front = header + b"".join(a[:6])
    want_len = REACH + 128 * 1024 + 4096
    big_at = len(front)
    end = big_at + want_len
    end += (-(end - (REACH - HEAD_BYTES))) % 65536            # end - (reach - 36) = a multiple of 64 KiB
    l_seq = (end - big_at - 36 - 7 - 4) * 2 // 3 - 2
    big = record(tid=0, pos=100000, name=b"bigger\x00", cigar=[op(l_seq, M)], seq=b"\x11" * ((l_seq + 1) // 2), qual=b"\x1e" * l_seq,
                 aux=b"\x1e" * (end - big_at - 36 - 7 - 4 - (l_seq + 1) // 2 - l_seq))
    assert big_at + len(big) == end
    big_case = Case("big/1M", 2, header, a[:6] + [big] + a[6:] + c)
    for shift in (-1, 0, 1):
        lens = tile(big_case.stream_len, 65536, first=65536 + shift)
        out.append(big_case.with_table("64K%+d" % shift, lens, notes=dict(big=len(big), big_end=end, shift=shift)))
    return out


def _tiny(tid, pos):
    return record(tid=tid, pos=pos, name=b"\x00")          # 37 bytes: a placed record with nothing but its fixed part


def family3():
    """65 536-byte blocks of nothing but 37-byte placed records: 1 772 begin in a block whose first record begins within its first
    eight bytes -- at its first byte, and with a record straddling in at the front."""
    header = bam_header(3, text_len=50)
    n = 3 * 1772 + 40
    recs = [_tiny(min(k * 3 // n, 2), 10 * k % 100000) for k in range(n)]
    base = Case("full", 3, header, recs)
    H, total = base.header_end, base.stream_len
    out = [base.with_table("aligned", tile(total, 65536, first=H), notes=dict(straddle=0)),
           base.with_table("straddle3", tile(total, 65536, first=H + 37 - 3), notes=dict(straddle=3)),
           base.with_table("straddle8", tile(total, 65536, first=H + 37 * 5 - 8), notes=dict(straddle=8))]
    return out


def family4():
    """Field extremes: CIGARs of 0, 1, 63, 64, 65 and 65 535 ops beginning in one block behind a hundred records with ops (more than
    one round of the wave extraction, the lanes' prefix sum with 65 535 in it); flag 0xFFFF, MAPQ 0 and 255; pos 0 and 2^31 - 2 with
    a 100 M-base M op; CIGARs without reference length; ops = and X, which alone decide reference 1's largest end."""
    rng = np.random.default_rng(404)
    header = bam_header(3, text_len=70)
    recs = []
    for k in range(100):
        n_cig = int(rng.integers(0, 6))
        recs.append(record(tid=0, pos=k, name=_name(rng, int(rng.integers(1, 9))), flag=int(rng.choice([0, 16, 0xFFFF])), mapq=int(rng.choice([0, 60, 255])),
                           cigar=[op(int(rng.integers(1, 50)), int(rng.choice([M, I, D, N, S, H, P, EQ, X]))) for _ in range(n_cig)]))
    recs.append(record(tid=0, pos=0, name=b"p0\x00", cigar=[op(5, M)], flag=0xFFFF, mapq=255))
    for n_cig in (0, 1, 63, 64, 65, 65535):
        recs.append(record(tid=0, pos=200 + n_cig, name=b"n%d\x00" % n_cig, mapq=0, cigar=[op(1 + j % 7, (M, I)[j % 2]) for j in range(n_cig)]))
    recs.append(record(tid=0, pos=300, name=b"allIS\x00", cigar=[op(7, S), op(9, I), op(3, S)], seq=b"\x21" * 10, qual=b"\x05" * 19))
    recs.append(record(tid=0, pos=(1 << 31) - 2, name=b"far\x00", cigar=[op(100_000_000, M)]))
    recs.append(record(tid=1, pos=1000, name=b"m\x00", cigar=[op(50, M)]))
    recs.append(record(tid=1, pos=1001, name=b"eqx\x00", cigar=[op(30, EQ), op(1, X), op(30, EQ), op(40, S)]))
    recs.append(record(tid=1, pos=1002, name=b"none\x00"))
    recs.append(record(tid=2, pos=(1 << 31) - 2, name=b"edge\x00"))
    recs += [record(tid=-1, pos=-1, name=b"u%d\x00" % k, flag=4) for k in range(5)]
    base = Case("extremes", 4, header, recs)
    return [base.with_table("64K", tile(base.stream_len, 65536), notes={}), base.with_table("48K", tile(base.stream_len, 0xC000, first=base.header_end), notes={})]


def family5():
    """References: three in one block, a tid beyond the header's references in the unplaced tail, reference ids going down inside a
    block and across two, and a tid window of (1, 2)."""
    rng = np.random.default_rng(505)
    header = bam_header(3, text_len=40)

    def run(tid, n, pos0=0):
        return [record(tid=tid, pos=pos0 + 7 * k if tid >= 0 else -1, name=_name(rng, int(rng.integers(2, 12))), cigar=[op(40, M), op(100 + k, N), op(20, M)] if tid >= 0 else [],
                       flag=0 if tid >= 0 else 4) for k in range(n)]
    r0, r1, r2, un = run(0, 30), run(1, 12), run(2, 30), run(-1, 12)
    beyond = record(tid=7, pos=5, name=b"beyond\x00", cigar=[op(10, M)])
    recs = r0 + r1 + r2 + un[:6] + [beyond] + un[6:]
    base = Case("refs", 5, header, recs)
    H = base.header_end
    len0, len1, len2 = (sum(len(r) for r in rr) for rr in (r0, r1, r2))
    three = [H + len0 - 3 * len(r0[-1]) - 5, 5 + 3 * len(r0[-1]) + len1 + 4 * len(r2[0]) + 11]
    three.append(base.stream_len - sum(three))
    out = [base.with_table("three_in_one", three, notes=dict(three=1, sorted=True)),
           base.with_table("window_1_2", three, tid_lo=1, tid_hi=2, notes=dict(sorted=True, window=True)),
           base.with_table("window_1_2/one_block", [base.stream_len], tid_lo=1, tid_hi=2, notes=dict(sorted=True, window=True))]
    down_in = Case("refs_down_inside", 5, header, r0[:8] + r2[:8] + r1[:8] + r2[8:16] + un[:3])
    out.append(down_in.with_table("one", [down_in.stream_len], notes=dict(sorted=False)))
    down_x = Case("refs_down_across", 5, header, r0[:8] + r2[:8] + r1[:8] + un[:3])
    cut = down_x.offsets[16]
    out.append(down_x.with_table("two", [cut, down_x.stream_len - cut], notes=dict(sorted=False)))
    return out


FILTERS = ((10, 0, 0), (0, 0x2, 0), (0, 0, 0x10), (30, 0x1, 0x400), (255, 0, 0), (0, 0xFFFF, 0))


def family6():
    """The read filter: each of its three values alone and together, over records of every MAPQ and flag."""
    rng = np.random.default_rng(606)
    header = bam_header(3, text_len=30)
    recs = _short_records(rng, 90, flags=(0, 16, 99, 147, 83, 163, 256, 1024, 0x401, 0xFFFF), mapqs=(0, 1, 9, 10, 11, 29, 30, 60, 254, 255))
    base = Case("filter", 6, header, recs)
    out = []
    for f in FILTERS:
        for L in (61, 4096):
            out.append(base.with_table("q%d_f%x_F%x/L%d" % (f + (L,)), tile(base.stream_len, L), filt=f, notes={}))
    return out


def family7():
    """The CG placeholder: a first op <l_seq>S with bytes behind QUAL is the host's; without bytes behind, or an S of another
    length, it is not."""
    header = bam_header(3, text_len=30)
    plain = [record(tid=0, pos=k, name=b"p%d\x00" % k, cigar=[op(30, M)]) for k in range(6)]

    def rec(s_len, aux):
        return record(tid=0, pos=50, name=b"cg\x00", cigar=[op(s_len, S), op(500, N)], seq=b"\x11" * 10, qual=b"\x1e" * 20, aux=aux)
    cg = b"CGBI" + struct.pack("<I", 2) + struct.pack("<2I", op(20, M), op(5, I))
    out = []
    for nm, r, want in (("placeholder", rec(20, cg), True), ("any_aux", rec(20, b"NMC\x00"), True), ("no_aux", rec(20, b""), False), ("other_S", rec(19, cg), False),
                        ("unplaced", record(tid=0, pos=-1, name=b"cg\x00", cigar=[op(20, S)], seq=b"\x11" * 10, qual=b"\x1e" * 20, aux=cg), False)):
        c = Case("cg/" + nm, 7, header, plain[:3] + [r] + plain[3:])
        out.append(c.with_table("one", [c.stream_len], notes=dict(needs_host=want)))
        out.append(c.with_table("L61", tile(c.stream_len, 61), notes=dict(needs_host=want)))
    return out


def family8():
    """Windows: one stream cut at offsets inside and between its last records -- 0, 1, 3, 4, 35, 36, 37 bytes into a record and a byte
    before its end --, with and without more behind, the buffer going on with the stream's own bytes or with random ones."""
    rng = np.random.default_rng(808)
    header = bam_header(3, text_len=30)
    recs = _short_records(rng, 40, n_ref=2)
    base = Case("window", 8, header, recs)
    cuts = []
    for k in (-1, -2, -3, -5):
        o, n = base.offsets[k], len(base.records[k])
        cuts += [o, o + 1, o + 3, o + 4, o + HEAD_BYTES - 1, o + HEAD_BYTES, o + HEAD_BYTES + 1, o + n - 1]
    out = []
    for cut in sorted(set(cuts)):
        for more in (1, 0):
            for junk in (None, 8000 + cut):
                out.append(base.with_table("at%d/more%d/%s" % (cut, more, "own" if junk is None else "junk"), tile(cut, 37), stream_len=cut, more=more, junk=junk,
                                           notes=dict(cut=cut)))
    return out


def family9():
    """Records that contradict themselves: block sizes below 32 (and exactly 32, which is none), fields beyond the block size, a
    stream that ends 1, 3, 4 and 35 bytes into a record."""
    rng = np.random.default_rng(909)
    header = bam_header(3, text_len=30)
    good = _short_records(rng, 16, n_ref=2)
    out = []
    bads = [("bs31", record(tid=0, pos=9, name=b"", l_name=0, block_size=31) + b"\x00" * 8, True), ("bs0", record(tid=0, pos=9, name=b"x\x00", block_size=0), True),
            ("bs32", record(tid=0, pos=9, name=b"", l_name=0), False),
            ("cigar_beyond", record(tid=0, pos=9, name=b"x\x00", cigar=[op(5, M)], n_cigar=2), True),
            ("name_beyond", record(tid=0, pos=9, name=b"x\x00", l_name=3), True),
            ("seq_beyond", record(tid=0, pos=9, name=b"x\x00", l_seq=1), True),
            ("l_seq_negative", record(tid=0, pos=9, name=b"x\x00", l_seq=-1, qual=b""), True)]
    for nm, bad, corrupt in bads:
        c = Case("bad/" + nm, 9, header, good[:8] + [bad] + good[8:], notes=dict(bad_index=8, corrupt=corrupt))
        out.append(c.with_table("one", [c.stream_len]))
        out.append(c.with_table("L61", tile(c.stream_len, 61)))
    whole = Case("bad/ends_inside", 9, header, good, notes=dict(bad_index=len(good) - 1, corrupt=True))
    for into in (1, 3, 4, 35):
        cut = whole.offsets[-1] + into
        out.append(whole.with_table("%d/one" % into, [cut], stream_len=cut, junk=9000 + into))
        out.append(whole.with_table("%d/L61" % into, tile(cut, 61), stream_len=cut, junk=9000 + into))
    return out


def family10():
    """Decoys: bytes inside a true record's QUAL that satisfy the rule, and a true record that does not."""
    rng = np.random.default_rng(1010)
    header = bam_header(3, text_len=30)
    good = _short_records(rng, 30, n_ref=1)
    good = [r for r in good if struct.unpack_from("<i", r, 4)[0] == 0]
    decoy = [record(tid=0, pos=70 + k, name=b"decoy%d\x00" % k, cigar=[op(9, M)]) for k in range(4)]
    out = []

    def host(payload, name):
        return record(tid=0, pos=4000, name=name, cigar=[op(len(payload), M)], seq=b"\xff" * ((len(payload) + 1) // 2), qual=payload)
    # four chained records fill the QUAL to its last byte: the guess of a block cut in front of them is the first decoy
    four = b"".join(decoy)
    t = host(four, b"four\x00")
    c = Case("decoy/four", 10, header, good[:5] + [t] + good[5:])
    q0 = c.offsets[5] + len(t) - len(four)
    out.append(c.with_table("cut", [q0 - 2, c.stream_len - q0 + 2], notes=dict(decoy_at={1: q0})))
    out.append(c.with_table("L61", tile(c.stream_len, 61, first=q0 - 2), notes=dict(decoy_from=q0, decoy_to=c.offsets[5] + len(t))))
    # three only: the chain fails behind the third
    three = b"".join(decoy[:3]) + b"\xff" * 60
    t = host(three, b"three\x00")
    c = Case("decoy/three", 10, header, good[:5] + [t] + good[5:])
    q0 = c.offsets[5] + len(t) - len(three)
    out.append(c.with_table("cut", [q0 - 2, c.stream_len - q0 + 2], notes=dict(decoy_at={})))
    # four, the last of them within 36 bytes of the stream's end: the chain is cut short there, whatever the fourth holds
    tail4 = b"".join(decoy[:3]) + decoy[3][:20]
    t = host(tail4, b"short\x00")
    c = Case("decoy/near_end", 10, header, good + [t])
    q0 = c.stream_len - len(tail4)
    out.append(c.with_table("cut", [q0 - 2, c.stream_len - q0 + 2], notes=dict(decoy_at={1: q0}, reason="a record contradicts itself")))   # (the walk from the decoy ends in the cut one)
    # a true record with a blank in its name: legal to walk, not plausible -- a block that begins with it guesses the one behind
    blank = record(tid=0, pos=4000, name=b"a b\x00", cigar=[op(30, M)])
    c = Case("decoy/blank_name", 10, header, good[:5] + [blank] + good[5:])
    q0 = c.offsets[5]
    out.append(c.with_table("cut", [q0, c.stream_len - q0], notes=dict(decoy_at={1: c.offsets[6]})))
    return out


def family11():
    """XS: spliced and unspliced reads with random aux areas, an area that ends exactly with the record, and behind the stream's
    last record pad bytes that spell a strand."""
    rng = np.random.default_rng(1111)
    header = bam_header(3, text_len=30)
    recs = _short_records(rng, 150, aux=xscases.random_area)
    k_last = max(k for k, r in enumerate(recs) if struct.unpack_from("<i", r, 4)[0] == 2)
    recs[k_last] = record(tid=2, pos=1 << 20, name=b"last\x00", cigar=[op(10, M), op(500, N), op(10, M)], aux=b"NHC\x01")   # no strand of its own
    recs = recs[:k_last + 1]
    recs.insert(5, record(tid=0, pos=3, name=b"star\x00", cigar=[op(10, M), op(500, N), op(10, M)], aux=xscases.star_area(b"-")))
    recs.insert(6, record(tid=0, pos=4, name=b"cut\x00", cigar=[op(10, M), op(500, N), op(10, M)], aux=b"NHC\x01XSA"))  # the value would lie in the next record
    base = Case("xs", 11, header, recs, tail=b"XSA-" * 8, notes=dict(tail=b"XSA-" * 8))
    n = base.stream_len - 32
    base.stream_len = n
    out = []
    for L in (37, 4096, 65536):
        out.append(base.with_table("L%d" % L, tile(n, L), notes=dict(tail=b"XSA-" * 8)))
    return out


FAMILIES = {1: family1, 2: family2, 3: family3, 4: family4, 5: family5, 6: family6, 7: family7, 8: family8, 9: family9, 10: family10, 11: family11}
_CASES = {}


def cases(family):
    if family not in _CASES:
        _CASES[family] = FAMILIES[family]()
        names = [c.name for c in _CASES[family]]
        assert len(set(names)) == len(names)
    return _CASES[family]


# ---- run tables for the bounds kernel --------------------------------------------------------------------------------------
def bounds_cases():
    """(n, run count, cap): tids in runs, n of 1, 255, 256, 257 and about 5 000 (the kernel's blocks are 256 lanes), run counts a cap
    less one, the cap and one more."""
    out = []
    for n in (1, 255, 256, 257, 5003):
        for cap in sorted({1, min(n, 7), min(n, 64)}):
            for runs in (cap - 1, cap, cap + 1):
                if 1 <= runs <= n:
                    out.append((n, runs, cap))
    return out


def bounds_input(n, runs, seed):
    rng = np.random.default_rng(seed)
    starts = np.sort(np.concatenate(([0], rng.choice(np.arange(1, n), runs - 1, replace=False)))) if runs > 1 else np.array([0])
    tid = np.zeros(n, np.int32)
    ids = rng.integers(0, 1 << 20, runs)
    ids[1:] = np.where(ids[1:] == ids[:-1], ids[1:] + 1, ids[1:])
    for k, s in enumerate(starts):
        tid[s:] = ids[k]
    assert all(s == 0 or tid[s] != tid[s - 1] for s in starts)
    cig_off = np.cumsum(rng.integers(0, 9, n + 1)).astype(np.uint32) + np.uint32(0xFFFF0000)   # (offsets that need all 32 bits)
    want = {(int(s), int(np.uint32(tid[s])) | (int(cig_off[s]) << 32)) for s in starts}
    return tid, cig_off, want
