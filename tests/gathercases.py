"""Sizes, inputs and expectations for the gather side of ``--anyOrder`` and the device-wide scan at the sizes production data has
(csrc/spl_sort.hip: ``spl_sort_make_keys_kernel``, ``spl_sort_gather_kernel``, ``spl_sort_cigar_kernel``, ``spl_dev_launch_sort_scan``).
The thresholds of ``spl_sam_last_newline_kernel`` (csrc/spl_sam.hip), which tests/test_gpu_sam_join.py runs, are here too.  No tests
in here, and nothing of the product: numpy only.

tests/test_gathercases_host.py proves that every named size lies on the side of its threshold that its name says, and holds the
restatements below against the wave emulator where that is quick; tests/test_gpu_sort_gather.py runs the kernels against them.
The reference has no counterpart: it reads a file that ``samtools sort`` has put in order (SpliSER_v0_1_8.py:422)."""
import numpy as np

TILE = 1024           # (splsort::TILE, spl_sort_wave.h: 16 rounds of 64 values)
MAX_PARTS = 2048      # (splsort::MAX_PARTS, spl_sort_wave.h: waves a launch; beyond this many tiles a wave walks several)
GATHER_BLOCK = 256    # (GATHER_BLOCK, spl_sort.hip: threads of a workgroup of make_keys, gather and cigar)
GATHER_GRID = 2048    # (GATHER_GRID, spl_sort.hip: the most workgroups of their grids; the loop takes the rest)

G1 = GATHER_GRID * GATHER_BLOCK   # 524 288: the most records that one trip of the gather's loops takes
S1 = MAX_PARTS * TILE             # 2 097 152: the most values that the scan takes with one tile a part

SCAN_SIZES = (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 64 * TILE + 1, S1, S1 + 1, 3 * S1 + 777)
SCAN_SMALL = tuple(n for n in SCAN_SIZES if n <= 64 * TILE + 1)      # (what the emulator walks in a moment)
SCAN_KINDS = ("mixed", "zeros", "ones")
GATHER_SIZES = (1, 255, 256, 257, G1, G1 + 1, 2 * G1 + 300)
NEWLINE_GROUPS = 2048  # (spl_dev_launch_sam_last_newline, spl_sam.hip: the most workgroups of its grid, 256 * 8; the loop takes the rest)
NEWLINE_ONE_TRIP = NEWLINE_GROUPS * 256 * 16    # 8 MiB: the text that one trip of last_newline's loop takes, a lane per sixteen bytes
NEWLINE_TEXT = NEWLINE_ONE_TRIP + 4096          # the text whose last 4 KiB are the second words of the first 256 lanes
FOUR_GIB = 1 << 32                              # offsets from here on have a high half
DECODE_RECORDS = 2_100_000        # above S1 (and G1): every kernel of RecordSort::run leaves its first trip


def plan(n, max_parts=MAX_PARTS):
    """splsort::plan_for in plain integers -> (tiles, tiles a part, parts)."""
    n_tiles = -(-n // TILE)
    want = min(n_tiles, max(max_parts, 1))
    if not want:
        return 0, 1, 0
    per = -(-n_tiles // want)
    return n_tiles, per, -(-n_tiles // per)


def gather_grid(n):
    """gather_grid of spl_sort.hip: workgroups of a launch over n records."""
    return min(-(-n // GATHER_BLOCK), GATHER_GRID)


def gather_trips(n):
    """-> (the trips of the thread that takes most, of the one that takes fewest) through the loop
    ``for (i = block * GATHER_BLOCK + thread; i < n; i += grid * GATHER_BLOCK)``."""
    step = gather_grid(n) * GATHER_BLOCK
    return -(-n // step), n // step


def newline_trips(lo, hi):
    """-> (the trips of the lane that takes most, of the one that takes fewest) through the loop of spl_sam_last_newline_kernel: a
    lane per 16-byte word of [lo & ~15, (hi + 15) & ~15), at most NEWLINE_GROUPS workgroups of 256 lanes."""
    words = (((hi + 15) & ~15) - (lo & ~15)) // 16
    step = min(-(-words // 256), NEWLINE_GROUPS) * 256
    return -(-words // step), words // step


# ---- the scan -----------------------------------------------------------------------------------------------------------------------

def scan_values(kind, n, seed=3):
    """n counts: 'mixed' -- 0..8, every seventh one 0 (a read without a CIGAR) --, 'zeros', 'ones', and 'full': 2047 each and the
    rest of 2^32 - 1 on the last one, so that the sums reach the largest 32-bit value and not one more."""
    if kind == "zeros":
        return np.zeros(n, np.uint32)
    if kind == "ones":
        return np.ones(n, np.uint32)
    if kind == "full":
        v = np.full(n, 2047, np.uint32)
        rest = (1 << 32) - 1 - 2047 * n
        assert n > 0 and 0 <= rest and 2047 + rest < (1 << 32)
        v[-1] += np.uint32(rest)
        return v
    assert kind == "mixed"
    v = np.random.default_rng(seed + n).integers(0, 9, n, dtype=np.uint32)
    v[::7] = 0
    return v


def scan_expected(v):
    """Inclusive prefix sums in 64 bits, cast down."""
    return np.cumsum(v, dtype=np.uint64).astype(np.uint32)


# ---- make_keys ----------------------------------------------------------------------------------------------------------------------

TOP = (1 << 31) - 1


def key_fields(n, seed=11):
    """-> (tid, pos), int32, drawn from the whole of [0, 2^31 - 1]; both ends are there, at the first and the last index and, where
    there is room, on both sides of every multiple of G1."""
    rng = np.random.default_rng(seed + n)
    tid = rng.integers(0, TOP + 1, n, dtype=np.int64)
    pos = rng.integers(0, TOP + 1, n, dtype=np.int64)
    at = [0, n - 1] + [k for m in range(G1, n + 1, G1) for k in (m - 1, m)]
    for j, k in enumerate(i for i in at if 0 <= i < n):
        tid[k], pos[k] = (TOP, 0) if j & 1 else (0, TOP)
    if n > 2:
        tid[1], pos[1] = TOP, TOP
    return tid.astype(np.int32), pos.astype(np.int32)


def keys_expected(tid, pos):
    return (tid.astype(np.uint64) << np.uint64(32)) | pos.astype(np.uint64)


# ---- gather and cigar ---------------------------------------------------------------------------------------------------------------

class GatherCase(object):
    """n records in file order, a permutation of them, and the keys of the sorted order (only their high words are read)."""

    def __init__(self, n, seed=21):
        rng = np.random.default_rng(seed + n)
        idx = np.arange(n, dtype=np.int64)
        self.n = n
        self.perm = rng.permutation(n).astype(np.uint32)
        self.pos = rng.integers(0, TOP + 1, n, dtype=np.int64).astype(np.int32)
        self.flag = (idx & 0xFFFF).astype(np.uint16)
        self.xs = np.array([0, ord("+"), ord("-")], np.uint8)[rng.integers(0, 3, n)]
        counts = rng.integers(1, 7, n, dtype=np.int64)
        counts[::7] = 0
        counts[rng.integers(0, n, min(n, 5))] = 1000
        self.counts = counts.astype(np.uint32)
        self.cig_off = np.concatenate(([0], np.cumsum(counts))).astype(np.uint32)
        total = int(self.cig_off[-1])
        owner = np.repeat(idx, counts)
        within = np.arange(total, dtype=np.int64) - np.repeat(self.cig_off[:-1].astype(np.int64), counts)
        self.cigar = (owner << 4 | within % 9).astype(np.uint32)          # (index << 4 | code: a misplaced run shows)
        self.tid_sorted = rng.integers(0, TOP + 1, n, dtype=np.int64)
        self.tid_sorted[[0, n - 1]] = (0, TOP) if n > 1 else (TOP,)
        self.keys = (self.tid_sorted.astype(np.uint64) << np.uint64(32)) | self.pos[self.perm].astype(np.uint32).astype(np.uint64)

    def expected(self):
        """-> dict: the fixed-size fields in the new order, cig_off_out before the scan (counts) and after it, the CIGAR runs."""
        p = self.perm.astype(np.int64)
        counts = self.counts[p].astype(np.int64)
        off = np.concatenate(([0], np.cumsum(counts, dtype=np.uint64))).astype(np.uint32)
        total = int(off[-1])
        owner = np.repeat(p, counts)
        within = np.arange(total, dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), counts)
        return dict(pos=self.pos[p], flag=self.flag[p], xs=self.xs[p], tid=self.tid_sorted.astype(np.int32),
                    counts=np.concatenate(([0], counts)).astype(np.uint32), cig_off=off,
                    cigar=self.cigar[self.cig_off[owner].astype(np.int64) + within])

    def expected_slowly(self, k):
        """Output record k the plain way -> (pos, flag, xs, CIGAR words): what ``expected`` is held against on the host."""
        j = int(self.perm[k])
        return int(self.pos[j]), int(self.flag[j]), int(self.xs[j]), self.cigar[int(self.cig_off[j]):int(self.cig_off[j + 1])].tolist()


# ---- the decode of a file above both thresholds -------------------------------------------------------------------------------------

BAM_RECORD = np.dtype([("block_size", "<i4"), ("tid", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_ops", "<u2"), ("flag", "<u2"),
                       ("l_seq", "<i4"), ("next_tid", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4"), ("name", "S2"), ("op", "<u4")])
DECODE_REFS = ["a", "b", "c"]


def decode_fields(n=DECODE_RECORDS, seed=31):
    """-> (tid, pos, flag, op): three references drawn at random (their records interleave), POS from 1..4096 (as the arrays keep it,
    1-based: ties dominate, and only a stable sort leaves them in file order), FLAG the index's low 16 bits, one M op of
    1 + index % 1000 bases."""
    rng = np.random.default_rng(seed)
    idx = np.arange(n, dtype=np.int64)
    tid = rng.integers(0, len(DECODE_REFS), n, dtype=np.int64).astype(np.int32)
    pos = rng.integers(1, 4097, n, dtype=np.int64).astype(np.int32)
    flag = (idx & 0xFFFF).astype(np.uint16)
    op = ((1 + idx % 1000) << 4).astype(np.uint32)
    return tid, pos, flag, op


def bam_records(tid, pos, flag, op):
    """The records as a BAM file holds them, one after the other (``ordercases.record``'s layout: name ``r\\0``, MAPQ 60, no sequence,
    one CIGAR op), made as one structured array."""
    r = np.zeros(len(tid), BAM_RECORD)
    assert BAM_RECORD.itemsize == 42
    r["block_size"], r["tid"], r["pos"], r["l_name"], r["mapq"], r["bin"], r["n_ops"], r["flag"] = 38, tid, pos - 1, 2, 60, 4680, 1, flag
    r["next_tid"], r["next_pos"], r["name"], r["op"] = -1, -1, b"r", op
    return r.tobytes()


def decode_expected(tid, pos, flag, op, t):
    """Reference t's reads: numpy's stable sort by POS of what was written -> (pos, flag, cig_off, cigar)."""
    mine = np.flatnonzero(tid == t)
    order = mine[np.argsort(pos[mine], kind="stable")]
    return pos[order], flag[order], np.arange(len(order) + 1, dtype=np.uint32), op[order]
