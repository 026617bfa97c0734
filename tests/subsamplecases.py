"""Shared by the tests of subsampling (``spl_reads_subsample``, ``saturation``, ``junctions --subsample``): the rule restated in
plain Python integers from the issue's text, a search for small integer keys that give any wanted keep / drop pattern at a
threshold -- keys go up directly (``upload_soa(with_keys=True)``), so a test says exactly which read is kept --, and the builders
of the cases the kernels are held to.  Nothing here imports the package's code or calls the library; nothing touches the GPU."""
import numpy as np

MASK = (1 << 64) - 1
ALL = 1 << 32                 # the threshold that keeps every read
M, I, N = 0, 1, 3             # BAM op codes


# ---- the rule -----------------------------------------------------------------------------------------------------------------
def draw(key, seed):
    z = (key ^ ((seed * 0x9e3779b97f4a7c15) & MASK)) & MASK
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK
    z ^= z >> 31
    return z >> 32


def nameless_key(pos, flag, n_ops):
    return ((pos & 0xffffffff) << 32) | ((flag & 0xffff) << 16) | (n_ops & 0xffff)


def keep(key, pos, flag, n_ops, seed, threshold):
    k = int(key) or nameless_key(int(pos), int(flag), int(n_ops))
    return draw(k, int(seed)) < int(threshold)


def keep_mask(keys, pos, flag, n_ops, seed, threshold):
    """-> bool[n], read by read."""
    return np.array([keep(k, p, f, o, seed, threshold) for k, p, f, o in zip(np.asarray(keys).tolist(), np.asarray(pos).tolist(), np.asarray(flag).tolist(),
                                                                             np.asarray(n_ops).tolist())], bool)


def thresholds(steps):
    return [(k << 32) // steps for k in range(1, steps + 1)]


def keys_for(pattern, seed, threshold, first=1):
    """Distinct small keys (from ``first`` up) under which read i is kept exactly where ``pattern[i]``."""
    if (threshold == 0 and any(pattern)) or (threshold >= ALL and not all(pattern)):
        raise ValueError("no key gives this pattern at this threshold")
    out, k = [], first
    kept, dropped = [], []
    for want in pattern:
        pool = kept if want else dropped
        while not pool:
            (kept if draw(k, seed) < threshold else dropped).append(k)
            k += 1
        out.append(pool.pop(0))
    return np.array(out, np.uint64)


# ---- reads --------------------------------------------------------------------------------------------------------------------
class Reads(object):
    """One segment's host arrays."""

    def __init__(self, pos, flag, cig_off, cigar, xs, keys):
        self.pos, self.flag = np.asarray(pos, np.int32), np.asarray(flag, np.uint16)
        self.cig_off, self.cigar = np.asarray(cig_off, np.uint32), np.asarray(cigar, np.uint32)
        self.xs, self.keys = np.asarray(xs, np.uint8), np.asarray(keys, np.uint64)
        self.n = int(self.pos.shape[0])

    @property
    def n_ops(self):
        return np.diff(self.cig_off.astype(np.int64))

    def masked(self, mask):
        """The reads where ``mask``, by numpy: what the device's selection has to equal."""
        mask = np.asarray(mask, bool)
        n_ops = self.n_ops
        op_mask = np.repeat(mask, n_ops)
        return Reads(self.pos[mask], self.flag[mask], np.concatenate(([0], np.cumsum(n_ops[mask]))), self.cigar[op_mask], self.xs[mask], self.keys[mask])

    def mask(self, seed, threshold):
        return keep_mask(self.keys, self.pos, self.flag, self.n_ops, seed, threshold)


OPS = {
    "plain": [(20, M)],
    "once": [(12, M), (80, N), (12, M)],
    "twice": [(10, M), (75, N), (9, M), (90, N), (10, M)],
    "none": [],
}


def long_ops(n_ops):
    """A CIGAR of n_ops ops: 2M 1I 2M 1I ... with one intron in the middle."""
    ops = [((2, M) if k % 2 == 0 else (1, I)) for k in range(n_ops)]
    ops[n_ops // 2 | 1] = (70 + n_ops % 7, N)
    ops[(n_ops // 2 | 1) - 1] = (15, M)
    ops[(n_ops // 2 | 1) + 1] = (15, M)
    return ops


def reads_of(kinds, keys, rng, flags=None, first_pos=100):
    """``kinds``: per read a name of OPS or a list of (length, op) -> Reads at ascending POS, flags of every pair kind unless given,
    strand bytes of all three values."""
    n = len(kinds)
    ops = [OPS[k] if isinstance(k, str) else k for k in kinds]
    counts = np.array([len(o) for o in ops], np.int64)
    cigar = np.array([(ln << 4) | op for o in ops for ln, op in o], np.uint32)
    pos = first_pos + 3 * np.arange(n)
    if flags is None:
        flags = rng.choice(np.array([0, 16, 99, 147, 83, 163, 99 | 256, 147 | 2048], np.uint16), n)
    xs = rng.choice(np.array([43, 45, 0], np.uint8), n)
    return Reads(pos, flags, np.concatenate(([0], np.cumsum(counts))), cigar, xs, keys)


def mixed_kinds(n, rng):
    return [("plain", "plain", "once", "plain", "twice", "once")[int(v)] for v in rng.integers(0, 6, n)]


# ---- the cases ----------------------------------------------------------------------------------------------------------------
SEED, HALF = 5, ALL // 2


def patterns(n, tile, rng):
    """-> [(name, bool[n])]: all, none, only the first, only the last, alternate, one run longer than a tile, random at 0.5."""
    out = [("all", np.ones(n, bool)), ("none", np.zeros(n, bool))]
    if n:
        first, last, alt = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
        first[0], last[-1], alt[::2] = True, True, True
        out += [("first", first), ("last", last), ("alternate", alt), ("random", rng.random(n) < 0.5)]
    if n > tile:
        run = np.zeros(n, bool)
        run[n - tile - 1:] = True          # (tile + 1 kept reads on end, across a tile's edge)
        run[0] = True
        out.append(("run", run))
    return out


def sizes(tile):
    return [0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1]


def size_cases(tile):
    """-> [(name, [Reads per segment], seed, threshold)] over every size and pattern, one segment each."""
    rng = np.random.default_rng(20261021)
    out = []
    for n in sizes(tile):
        for name, pattern in patterns(n, tile, rng):
            keys = keys_for(pattern, SEED, HALF, first=1 + 7 * n)
            out.append(("n%d_%s" % (n, name), [reads_of(mixed_kinds(n, rng), keys, rng)], SEED, HALF))
    return out


def cigar_cases(tile):
    rng = np.random.default_rng(7)
    out = []
    n = 2 * tile + 3
    for name, kept in (("kept", True), ("dropped", False)):      # reads without an op at a tile's first and last place
        kinds = mixed_kinds(n, rng)
        pattern = rng.random(n) < 0.5
        for at in (0, tile - 1, tile, 2 * tile - 1, 2 * tile, n - 1):
            kinds[at], pattern[at] = "none", kept
        out.append(("no_ops_%s" % name, [reads_of(kinds, keys_for(pattern, SEED, HALF, 11), rng)], SEED, HALF))
    for n_long in (300, 5000):                                    # one long CIGAR across a tile's edge, among reads of one op
        for kept in (True, False):
            kinds = ["plain"] * n
            pattern = rng.random(n) < 0.5
            at = tile - 1
            kinds[at], kinds[at + 1], pattern[at], pattern[at + 1] = long_ops(n_long), long_ops(9), kept, True
            pattern[at - 1] = True
            out.append(("long_%d_%s" % (n_long, "kept" if kept else "dropped"), [reads_of(kinds, keys_for(pattern, SEED, HALF, 3), rng)], SEED, HALF))
    return out


def segment_cases(tile):
    rng = np.random.default_rng(9)

    def seg(n, pattern=None, first=1):
        pattern = rng.random(n) < 0.5 if pattern is None else pattern
        return reads_of(mixed_kinds(n, rng), keys_for(pattern, SEED, HALF, first), rng)
    out = [("empty_middle", [seg(70), seg(0), seg(tile + 9, first=500)], SEED, HALF),
           ("loses_every_read", [seg(40), seg(130, np.zeros(130, bool), first=900), seg(66, first=4000)], SEED, HALF),
           ("boundary_in_a_tile", [seg(tile // 2 + 5), seg(tile + 1, first=9000), seg(3, first=50000)], SEED, HALF)]
    # a key of 0: the decision is by (POS, FLAG, ops); and pairs under random 64-bit keys, so that mates are kept together
    n = tile + 77
    kinds = mixed_kinds(n, rng)
    keys = np.zeros(n, np.uint64)
    keys[1::3] = rng.integers(1, 2 ** 63, len(keys[1::3]), dtype=np.uint64)
    out.append(("key_0", [reads_of(kinds, keys, rng)], SEED, HALF))
    n = 2 * tile + 10
    pair_keys = rng.integers(1, 2 ** 63, n // 2, dtype=np.uint64) << np.uint64(1)
    where = rng.permutation(n)
    keys, flags = np.empty(n, np.uint64), np.empty(n, np.uint16)
    keys[where[:n // 2]], keys[where[n // 2:]] = pair_keys, pair_keys
    flags[where[:n // 2]], flags[where[n // 2:]] = 99, 147
    out.append(("pairs", [reads_of(mixed_kinds(n, rng), keys, rng, flags=flags)], 12345, (3 * ALL) // 5))
    return out


def all_cases(tile):
    return size_cases(tile) + cigar_cases(tile) + segment_cases(tile)
