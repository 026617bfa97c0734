"""Inputs and expectations for the ``--anyOrder`` tests (``spl_bam_set_any_order``).  No tests in here.

A small pure-Python BAM writer that puts given records into BGZF blocks in ANY order (SAM specification section 4.2; ``struct`` +
``zlib``, nothing of the product), a shuffle of a workload's reads into it, and the expectation in numpy: every reference's reads
sorted by (POS, place in the file) with a stable argsort.  The reference has no counterpart: it reads through ``samtools view BAM
region`` (SpliSER_v0_1_8.py:422), which needs a coordinate-sorted, indexed file."""
import struct
import zlib

import numpy as np

from spliser_amd import samio

EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def bgzf(raw, level=1, block=0xff00):
    out = bytearray()
    for a in range(0, len(raw), block):
        chunk = raw[a:a + block]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = c.compress(chunk) + c.flush()
        out += struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(body) + 25)
        out += body + struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return bytes(out)


def record(tid, pos, flag, mapq, ops, aux=b""):
    """One alignment record.  ``pos``: 1-based, as a ReadSet keeps it (0: no position); ``ops``: CIGAR words (len << 4 | code)."""
    ops = np.asarray(ops, "<u4")
    name = b"r\0"
    return struct.pack("<iiiBBHHHiiii", 32 + len(name) + 4 * len(ops) + len(aux), tid, int(pos) - 1, len(name), int(mapq), 4680, len(ops), int(flag), 0, -1, -1, 0) \
        + name + ops.tobytes() + aux


def write_bam(path, names, lengths, records, so="unsorted", level=1, block=0xff00):
    """``records``: (tid, pos, flag, mapq, ops, aux) tuples, written in the order given, whatever that is.  ``so``: the header's
    ``@HD SO:`` value (``None``: no @HD line)."""
    text = "@HD\tVN:1.6\tSO:%s\n" % so if so is not None else ""
    head = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(names))
    for n, ln in zip(names, lengths):
        head += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", int(ln))
    with open(path, "wb") as fh:
        fh.write(bgzf(head, level, block))
        fh.write(bgzf(b"".join(record(*r) for r in records), level, block))
        fh.write(EOF_BLOCK)


def records_of(sets, tags=None, mapq=None):
    """The reads of ``sets`` (a ReadSet or None per reference id) as records in coordinate order.  ``tags``: per reference a list of
    aux areas, a read's own; ``mapq``: per reference an array (60 otherwise)."""
    out = []
    for tid, rs in enumerate(sets):
        if rs is None:
            continue
        off = np.asarray(rs.cig_off, np.int64)
        for k in range(rs.n):
            out.append((tid, int(rs.pos[k]), int(rs.flag[k]), int(mapq[tid][k]) if mapq is not None else 60, np.asarray(rs.cigar[off[k]:off[k + 1]], np.uint32),
                        tags[tid][k] if tags is not None else b""))
    return out


def shuffled(records, seed):
    """The same records in an order drawn from ``seed``."""
    order = np.random.default_rng(seed).permutation(len(records))
    return [records[i] for i in order]


def shuffle_workload(wl, path_sorted, path_shuffled, seed, tags=None):
    """The reads of a ``synth.Workload`` twice: in coordinate order (``SO:coordinate``) and shuffled by ``seed`` (``SO:unsorted``),
    both through this writer, MAPQ drawn from 0..60 by ``seed`` (so that a MAPQ filter has something to drop).  -> the records in
    the shuffled file's order."""
    rng = np.random.default_rng(seed + 1000)
    recs = records_of(wl.reads, tags=tags, mapq=[rng.integers(0, 61, rs.n) for rs in wl.reads])
    write_bam(path_sorted, wl.genome.chrom_names, wl.genome.chrom_lengths, recs, so="coordinate")
    mixed = shuffled(recs, seed)
    write_bam(path_shuffled, wl.genome.chrom_names, wl.genome.chrom_lengths, mixed, so="unsorted")
    return mixed


def placed(r, n_ref, read_filter=(0, 0, 0)):
    tid, pos, flag, mapq = r[0], r[1], r[2], r[3]
    q, need, drop = read_filter
    return 0 <= tid < n_ref and pos >= 1 and not (flag & drop) and (flag & need) == need and mapq >= q


def expected(records, n_ref, read_filter=(0, 0, 0), any_order=True):
    """What the decode of a file holding ``records`` in this order must hand out per reference id -> {tid: (ReadSet, [aux])}: the
    placed records of the reference in file order, and under ``any_order`` sorted by POS with numpy's stable argsort -- ties in
    file order."""
    out = {}
    for tid in range(n_ref):
        mine = [r for r in records if r[0] == tid and placed(r, n_ref, read_filter)]
        if any_order:
            order = np.argsort(np.array([r[1] for r in mine], np.int64), kind="stable")
            mine = [mine[i] for i in order]
        off = np.concatenate(([0], np.cumsum([len(r[4]) for r in mine]))).astype(np.int64)
        cigar = np.concatenate([np.asarray(r[4], np.int64) for r in mine]) if mine and off[-1] else np.zeros(0, np.int64)
        out[tid] = (samio.ReadSet(np.array([r[1] for r in mine], np.int64), np.array([r[2] for r in mine], np.int64), off, cigar), [r[5] for r in mine])
    return out


def same_reads(got, want):
    """A decoded ReadSet (or None / empty) against an expected one: every array equal."""
    n = 0 if got is None else got.n
    if n != want.n:
        return False
    if n == 0:
        return True
    return bool(np.array_equal(got.pos, want.pos) and np.array_equal(got.flag, want.flag) and np.array_equal(np.asarray(got.cig_off, np.int64), np.asarray(want.cig_off, np.int64))
                and np.array_equal(np.asarray(got.cigar, np.int64), np.asarray(want.cigar, np.int64)))


def multiset(rs, xs=None):
    """The reads of a ReadSet as a sorted list of (POS, FLAG, CIGAR words, strand byte): what does not depend on their order."""
    if rs is None or rs.n == 0:
        return []
    off = np.asarray(rs.cig_off, np.int64)
    return sorted((int(rs.pos[k]), int(rs.flag[k]), tuple(int(x) for x in rs.cigar[off[k]:off[k + 1]]), int(xs[k]) if xs is not None else 0) for k in range(rs.n))


def sort_cases(tile):
    """(name, keys, key_bits) for the sort itself, whose tile is ``tile`` keys (splsort::TILE): the list the emulator test
    (tests/test_sort_wave_host.py) and the device test (tests/test_gpu_any_order.py) both run against numpy's stable argsort."""
    rng = np.random.default_rng(20261018)
    cases = []
    for n in (0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 5):
        cases.append(("n=%d" % n, rng.integers(0, 1 << 40, n, dtype=np.uint64), 40))
    n = 3 * tile + 5
    cases.append(("all equal", np.full(n, 0x0000000300001234, np.uint64), 40))
    cases.append(("top digit of the tid only", (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(56)) | np.uint64(77), 64))
    cases.append(("lowest digit of the pos only", rng.integers(0, 256, n, dtype=np.uint64) | np.uint64(5 << 32 | 0x123400), 40))
    cases.append(("sorted", np.sort(rng.integers(0, 1 << 40, n, dtype=np.uint64)), 40))
    cases.append(("reverse sorted", np.sort(rng.integers(0, 1 << 40, n, dtype=np.uint64))[::-1].copy(), 40))
    for bits in (1, 8, 9, 33, 40, 63):
        cases.append(("key_bits=%d" % bits, rng.integers(0, 1 << bits, 2 * tile + 77, dtype=np.uint64), bits))
    return cases
