"""Alignment I/O on the host: SoA read sets, a SAM-text reader and a BAM/BGZF writer.

The GPU path consumes, per chromosome, exactly the three SAM columns ``checkBam`` reads from each
line ``samtools view`` prints (flag, POS, CIGAR -- SpliSER_v0_1_8.py:434-437) as structure-of-arrays
(``include/spliser.h``: ``spl_reads``).  Production input is BAM, decoded by the native reader in
``csrc/bam_reader.cpp`` (see ``native.BamFile``).  This module adds

  * ``read_sam``   -- a plain SAM-text reader (small inputs, fixtures; ``samtools view`` accepts SAM too), gzip'd or BGZF text too,
  * ``write_bam``  -- a spec-conformant BGZF/BAM writer used to make test and synthetic BAM files
                      (the image has no samtools/htslib), and ``write_sam`` for their text twins.
"""
import gzip
import re
import struct
import zlib

import numpy as np

__all__ = ["ReadSet", "read_sam", "write_bam", "write_sam", "cigar_ops", "cigar_string", "name_key", "OP_CODES"]

OP_CODES = "MIDNSHP=XB"
_CIGAR_RE = re.compile(r"(\d+)([MIDNSHP=XB])")
_OP_OF = {c: i for i, c in enumerate(OP_CODES)}


def cigar_ops(cigar):
    """'50M100N50M' -> [50<<4|0, 100<<4|3, 50<<4|0]; '*' -> []."""
    if cigar == "*":
        return []
    return [(int(n) << 4) | _OP_OF[c] for n, c in _CIGAR_RE.findall(cigar)]


def cigar_string(ops):
    return "".join("%d%s" % (int(o) >> 4, OP_CODES[int(o) & 15]) for o in ops) or "*"


_MASK64 = (1 << 64) - 1


def name_key(name):
    """The name key of a QNAME (bytes) by the library's rule (``csrc/spl_mate_rule.h``): FNV-1a over the bytes, then a 64-bit
    finisher; 0 for an empty name and for ``*`` ("no name"), 1 for another name whose hash comes to 0."""
    name = bytes(name)
    if name == b"" or name == b"*":
        return 0
    h = 0xcbf29ce484222325
    for b in name:
        h = ((h ^ b) * 0x100000001b3) & _MASK64
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & _MASK64
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & _MASK64
    h ^= h >> 33
    return h or 1


class ReadSet(object):
    """Reads of one chromosome in file order (SoA).  ``pos`` is 1-based (SAM POS).  ``xs``: None, or a strand byte per read
    (``'+'``, ``'-'``, 0) from the aligner's XS:A tag where the reader was asked for it (``read_sam(aux_strand=True)``,
    ``native.BamFile.set_aux_strand``).  ``name_key``: None, or the reads' name keys (uint64; ``name_key``) where the reader was
    asked for them (``read_sam(mate_keys=True)``, a decode with ``mate_keys``)."""
    __slots__ = ("pos", "flag", "cig_off", "cigar", "max_end", "xs", "name_key")

    def __init__(self, pos, flag, cig_off, cigar, max_end=None, xs=None, name_key=None):
        self.xs = None if xs is None else np.ascontiguousarray(xs, dtype=np.uint8)
        self.name_key = None if name_key is None else np.ascontiguousarray(name_key, dtype=np.uint64)
        self.pos = np.ascontiguousarray(pos, dtype=np.int32)
        self.flag = np.ascontiguousarray(flag, dtype=np.uint16)
        self.cig_off = np.ascontiguousarray(cig_off, dtype=np.uint32)
        self.cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
        if max_end is None:
            max_end = self._max_end()
        self.max_end = int(max_end)

    @property
    def n(self):
        return int(self.pos.shape[0])

    def _max_end(self):
        if self.n == 0:
            return 0
        code = self.cigar & 15
        length = (self.cigar >> 4).astype(np.int64)
        consumes = (code == 0) | (code == 2) | (code == 3) | (code == 7) | (code == 8)
        csum = np.concatenate(([0], np.cumsum(np.where(consumes, length, 0))))
        ref_len = csum[self.cig_off[1:].astype(np.int64)] - csum[self.cig_off[:-1].astype(np.int64)]
        return int((self.pos.astype(np.int64) + np.maximum(ref_len, 1) - 1).max())

    def take(self, lo, hi):
        """Reads [lo, hi) as a ReadSet of their own (views where the arrays allow; the CIGAR offsets begin at 0 again; the bound on
        their ends is the whole set's, which it cannot exceed)."""
        lo, hi = max(0, int(lo)), min(self.n, int(hi))
        if hi <= lo:
            return ReadSet.empty()
        o0, o1 = int(self.cig_off[lo]), int(self.cig_off[hi])
        off = self.cig_off[lo:hi + 1] if o0 == 0 else (self.cig_off[lo:hi + 1].astype(np.int64) - o0).astype(np.uint32)
        return ReadSet(self.pos[lo:hi], self.flag[lo:hi], off, self.cigar[o0:o1], max_end=self.max_end, name_key=None if self.name_key is None else self.name_key[lo:hi])

    @classmethod
    def empty(cls):
        return cls(np.zeros(0, np.int32), np.zeros(0, np.uint16), np.zeros(1, np.uint32), np.zeros(0, np.uint32), 0)

    @classmethod
    def from_records(cls, records):
        """records: iterable of (flag, pos, cigar_string)."""
        pos, flag, off, ops = [], [], [0], []
        for f, p, c in records:
            pos.append(p)
            flag.append(f)
            ops.extend(cigar_ops(c))
            off.append(len(ops))
        return cls(np.asarray(pos, np.int64), np.asarray(flag, np.int64), np.asarray(off, np.int64),
                   np.asarray(ops, np.int64))


def sam_aux_strand(cigar, optional):
    """The strand byte of one SAM line by the BAM decoder's rule (``spl_bam_set_aux_strand``): 0 unless the CIGAR holds an N op;
    else the value of the first optional column ``XS:A:`` if it is ``+`` or ``-`` (an ``XS:i:`` is another field), else 0."""
    if "N" not in cigar:
        return 0
    for field in optional:
        if field.startswith("XS:A:"):
            v = field[5:].rstrip("\n")
            return ord(v) if v in ("+", "-") else 0
    return 0


def read_sam(path, min_mapq=0, require_flags=0, exclude_flags=0, counts=None, aux_strand=False, mate_keys=False):
    """Parse SAM text (plain, or compressed as gzip / BGZF) -> (ref_names, {chrom: ReadSet}).  Keeps every record that has an RNAME, file order -- what ``samtools
    view`` would print; ``min_mapq`` / ``require_flags`` / ``exclude_flags`` are its -q / -f / -F on columns 5 and 2 (the BAM
    decoder's rule, ``spl_bam_set_filter``: flags first, MAPQ as a number).  ``counts``: a list that gets [records seen, dropped
    by flags, dropped by MAPQ] added to its three entries.  ``aux_strand``: every ReadSet gets ``xs`` (``sam_aux_strand``).  ``mate_keys``: every
    ReadSet gets ``name_key``, the key of column 1 as the file's bytes have it (the text is then read byte for byte, as Latin-1)."""
    names, per = [], {}
    seen = by_flags = by_mapq = 0
    with open(path, "rb") as handle:
        packed = handle.read(2) == b"\x1f\x8b"      # (gzip, or BGZF, which is gzip in many members)
    enc = dict(encoding="latin-1") if mate_keys else {}
    with (gzip.open(path, "rt", **enc) if packed else open(path, "r", **enc)) as handle:      # (both translate newlines alike: a carriage return ends a line)
        for line in handle:
            if line.startswith("@"):
                if line.startswith("@SQ"):
                    for field in line.rstrip("\n").split("\t")[1:]:
                        if field.startswith("SN:"):
                            names.append(field[3:])
                continue
            cols = line.split("\t")
            seen += 1
            if len(cols) < 6 or cols[2] == "*":
                continue
            flag = int(cols[1])
            if int(cols[3]) >= 1:      # (a record without a position is nobody's to filter: the BAM decoder's rule)
                if flag & exclude_flags or flag & require_flags != require_flags:
                    by_flags += 1
                    continue
                if int(cols[4]) < min_mapq:
                    by_mapq += 1
                    continue
            rec = per.get(cols[2])
            if rec is None:
                rec = per[cols[2]] = ([], [], [0], [], [], [])
                if cols[2] not in names:
                    names.append(cols[2])
            rec[0].append(int(cols[3]))
            rec[1].append(flag)
            rec[3].extend(cigar_ops(cols[5].strip()))
            rec[2].append(len(rec[3]))
            if aux_strand:
                rec[4].append(sam_aux_strand(cols[5], cols[11:]))
            if mate_keys:
                rec[5].append(name_key(cols[0].encode("latin-1")))
    sets = {c: ReadSet(np.asarray(p, np.int64), np.asarray(f, np.int64), np.asarray(o, np.int64),
                       np.asarray(g, np.int64), xs=np.asarray(x, np.uint8) if aux_strand else None, name_key=np.asarray(k, np.uint64) if mate_keys else None)
            for c, (p, f, o, g, x, k) in per.items()}
    if counts is not None:
        for k, v in enumerate((seen, by_flags, by_mapq)):
            counts[k] += v
    return names, sets


def _mapq_of(mapq, k_chrom, rs):
    """The MAPQ column of one entry of chrom_reads: 60 for every read, or the caller's array for that entry."""
    if mapq is None:
        return None
    m = np.asarray(mapq[k_chrom])
    if m.shape != (rs.n,) or (rs.n and (int(m.min()) < 0 or int(m.max()) > 255)):
        raise ValueError("mapq: one value in 0..255 per read of every entry of chrom_reads")
    return m


def _names_of(names, chrom_reads):
    if names is not None and (len(names) != len(chrom_reads) or any(len(t) != rs.n for t, (_, rs) in zip(names, chrom_reads))):
        raise ValueError("names: one bytes object per read of every entry of chrom_reads")
    return names


def write_sam(path, ref_names, ref_lengths, chrom_reads, mapq=None, names=None):
    """chrom_reads: list of (chrom, ReadSet) in file order.  mapq: per entry of chrom_reads an array of the reads' MAPQ (default:
    60 for every read).  names: per entry of chrom_reads a list of the reads' QNAMEs as bytes, written as they are (default:
    ``r<serial>``)."""
    names = _names_of(names, chrom_reads)
    with open(path, "w", **(dict(encoding="latin-1", newline="\n") if names is not None else {})) as fh:
        fh.write("@HD\tVN:1.6\tSO:coordinate\n")
        for n, ln in zip(ref_names, ref_lengths):
            fh.write("@SQ\tSN:%s\tLN:%d\n" % (n, ln))
        i = 0
        for k_chrom, (chrom, rs) in enumerate(chrom_reads):
            mq = _mapq_of(mapq, k_chrom, rs)
            for k in range(rs.n):
                ops = rs.cigar[rs.cig_off[k]:rs.cig_off[k + 1]]
                qname = "r%d" % i if names is None else bytes(names[k_chrom][k]).decode("latin-1")
                fh.write("%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t*\t*\n" % (qname, rs.flag[k], chrom, rs.pos[k], 60 if mq is None else mq[k], cigar_string(ops)))
                i += 1


# ---------------------------------------------------------------------------------------------------
# BGZF / BAM writer (SAM spec section 4): enough of the format for htslib-compatible files.

_BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_BGZF_BLOCK = 0xFF00  # uncompressed payload per block (< 64 KiB)


def _bgzf_block(payload, level):
    comp = zlib.compressobj(level, zlib.DEFLATED, -15)
    data = comp.compress(payload) + comp.flush()
    bsize = len(data) + 25  # total block size - 1
    if bsize > 0xFFFF:
        raise ValueError("BGZF block too large")
    header = struct.pack("<BBBBIBBHBBHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 0x42, 0x43, 2, bsize)
    return header + data + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload) & 0xFFFFFFFF)


def _reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def write_bam(path, ref_names, ref_lengths, chrom_reads, level=1, with_seq=False, unplaced=0, long_cigar_tag=False, mapq=None, tags=None, names=None):
    """Write a BAM file.  chrom_reads: list of (chrom, ReadSet) in file order.

    with_seq       -- emit a dummy SEQ/QUAL of the query length (realistic record size) instead of '*'
    unplaced       -- append this many records without a reference (tid -1) at the end
    long_cigar_tag -- store every CIGAR with more than 3 ops the way htslib stores >65535-op CIGARs:
                      a placeholder ``<qlen>S<rlen>N`` in the record and the real ops in a CG:B,I tag
    mapq           -- per entry of chrom_reads an array of the reads' MAPQ (default: 60 for every read)
    tags           -- per entry of chrom_reads a list of raw aux bytes per read (``b"XSA+"``, ...), appended to the record as
                      they are, behind the CG tag where there is one (default: no tags of the caller's)
    names          -- per entry of chrom_reads a list of the reads' QNAMEs as bytes, at most 254 each, without the NUL (default:
                      ``r<serial>``)
    """
    names = _names_of(names, chrom_reads)
    if tags is not None and (len(tags) != len(chrom_reads) or any(len(t) != rs.n for t, (_, rs) in zip(tags, chrom_reads))):
        raise ValueError("tags: one bytes object per read of every entry of chrom_reads")
    tid_of = {n: i for i, n in enumerate(ref_names)}
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in zip(ref_names, ref_lengths))
    head = [b"BAM\x01", struct.pack("<i", len(text)), text.encode("ascii"), struct.pack("<i", len(ref_names))]
    for n, ln in zip(ref_names, ref_lengths):
        nb = n.encode("ascii") + b"\x00"
        head += [struct.pack("<i", len(nb)), nb, struct.pack("<i", ln)]
    buf = bytearray(b"".join(head))
    with open(path, "wb") as fh:
        def flush(final=False):
            nonlocal buf
            while len(buf) >= _BGZF_BLOCK or (final and len(buf)):
                fh.write(_bgzf_block(bytes(buf[:_BGZF_BLOCK]), level))
                del buf[:_BGZF_BLOCK]

        serial = 0
        for k_chrom, (chrom, rs) in enumerate(chrom_reads):
            tid = tid_of[chrom]
            mq = _mapq_of(mapq, k_chrom, rs)
            for k in range(rs.n):
                ops = [int(o) for o in rs.cigar[rs.cig_off[k]:rs.cig_off[k + 1]]]
                qlen = sum(o >> 4 for o in ops if (o & 15) in (0, 1, 4, 7, 8))
                rlen = sum(o >> 4 for o in ops if (o & 15) in (0, 2, 3, 7, 8))
                name = (("r%d" % serial).encode("ascii") if names is None else bytes(names[k_chrom][k])) + b"\x00"
                if len(name) > 255:
                    raise ValueError("a QNAME has at most 254 bytes")
                serial += 1
                pos0 = int(rs.pos[k]) - 1
                aux = b""
                rec_ops = ops
                l_seq = qlen if with_seq else 0
                if long_cigar_tag and len(ops) > 3:
                    rec_ops = [(qlen << 4) | 4, (rlen << 4) | 3]   # htslib: <l_seq>S<rlen>N placeholder
                    aux = b"NMC\x00" + b"CGBI" + struct.pack("<i", len(ops)) + struct.pack("<%dI" % len(ops), *ops)
                    l_seq = qlen
                seq = bytes([0x11]) * ((l_seq + 1) // 2)
                qual = bytes([30]) * l_seq
                flag = int(rs.flag[k])
                end0 = pos0 + (rlen if (rlen and not flag & 4) else 1)
                body = struct.pack("<iiBBHHHiiii", tid, pos0, len(name), 60 if mq is None else int(mq[k]), _reg2bin(pos0, end0), len(rec_ops), flag,
                                   l_seq, -1, -1, 0) + name + struct.pack("<%dI" % len(rec_ops), *rec_ops) + seq + qual + aux + (bytes(tags[k_chrom][k]) if tags is not None else b"")
                buf += struct.pack("<i", len(body)) + body
                if len(buf) >= _BGZF_BLOCK:
                    flush()
        for k in range(unplaced):
            name = ("u%d" % k).encode("ascii") + b"\x00"
            body = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 0, 4680, 0, 4, 0, -1, -1, 0) + name
            buf += struct.pack("<i", len(body)) + body
        flush(final=True)
        fh.write(_BGZF_EOF)
