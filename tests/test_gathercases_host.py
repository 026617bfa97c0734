"""tests/gathercases.py without a GPU: every named size lies on the side of its threshold that its name says (the plan from the
emulator library's ``sort_wave_parts`` and the arithmetic of splsort::plan_for, the trips of the gather's grid-stride loops), the
numpy restatements that tests/test_gpu_sort_gather.py holds the kernels against agree with the wave emulator's scan and with a few
lines of plain Python, and the records of the large decode are laid out as ``ordercases.record`` lays them out."""
import ctypes

import numpy as np

import gathercases as G
import ordercases as O
from test_sort_wave_host import _ptr, lib  # noqa: F401  (the emulator library's fixture)


def test_the_constants_are_the_emulator_librarys(lib):
    assert lib.sort_wave_tile() == G.TILE
    assert G.G1 == 524288 and G.S1 == 2097152
    assert G.DECODE_RECORDS > G.S1 > G.G1


def test_every_scan_size_lies_where_its_name_says(lib):
    def parts(n):
        got = lib.sort_wave_parts(ctypes.c_uint64(n), ctypes.c_uint32(G.MAX_PARTS))
        assert got == G.plan(n)[2], n
        return got
    assert G.plan(G.S1) == (2048, 1, 2048) and parts(G.S1) == 2048                 # the last size with one tile a part
    assert G.plan(G.S1 + 1) == (2049, 2, 1025) and parts(G.S1 + 1) == 1025         # one value more: two tiles a part, the last part one
    assert G.plan(3 * G.S1 + 777) == (6145, 4, 1537) and parts(3 * G.S1 + 777) == 1537
    assert G.plan(G.DECODE_RECORDS)[1] == 2
    # digit_scan walks the parts' sums 64 a round: its second round begins at the 65th part
    assert G.plan(64 * G.TILE) == (64, 1, 64) and G.plan(64 * G.TILE + 1) == (65, 1, 65) and parts(64 * G.TILE + 1) == 65
    for n in G.SCAN_SIZES:
        n_tiles, per, p = G.plan(n)
        assert parts(n) == p
        assert (per == 1) == (n <= G.S1) and p <= G.MAX_PARTS
        assert n == 0 or (p - 1) * per < n_tiles <= p * per                          # (no part is empty)
    assert {0, 1, 63, 64, 65, G.TILE - 1, G.TILE, G.TILE + 1, 64 * G.TILE + 1, G.S1, G.S1 + 1, 3 * G.S1 + 777} == set(G.SCAN_SIZES)


def test_every_gather_size_lies_where_its_name_says():
    assert G.gather_grid(G.G1) == G.GATHER_GRID and G.gather_trips(G.G1) == (1, 1)        # every thread once, none twice
    assert G.gather_grid(G.G1 + 1) == G.GATHER_GRID and G.gather_trips(G.G1 + 1) == (2, 1)  # one thread goes round again
    assert G.gather_trips(2 * G.G1 + 300) == (3, 2)
    assert G.gather_trips(G.DECODE_RECORDS) == (5, 4)
    for n in (1, 255, 256, 257):
        assert G.gather_grid(n) == -(-n // 256) and G.gather_trips(n) == (1, 0 if n % 256 else 1)
    assert set(G.GATHER_SIZES) == {1, 255, 256, 257, G.G1, G.G1 + 1, 2 * G.G1 + 300}
    # the loop as the kernels write it, thread by thread, for the two sizes at the threshold
    for n in (G.G1, G.G1 + 1):
        first = np.arange(G.gather_grid(n) * G.GATHER_BLOCK, dtype=np.int64)
        trips = np.zeros(len(first), np.int64)
        i = first.copy()
        while (i < n).any():
            trips += i < n
            i += len(first)
        assert (int(trips.max()), int(trips.min())) == G.gather_trips(n) and int(trips.sum()) == n


def test_the_join_kernels_sizes_lie_where_their_names_say():
    assert G.NEWLINE_ONE_TRIP == 8 << 20 and G.NEWLINE_TEXT == (8 << 20) + 4096
    assert G.newline_trips(0, G.NEWLINE_ONE_TRIP) == (1, 1)                 # 8 MiB: every lane one word
    assert G.newline_trips(0, G.NEWLINE_ONE_TRIP + 1) == (2, 1)             # one byte more: lane 0 takes a second
    assert G.newline_trips(0, G.NEWLINE_TEXT) == (2, 1)
    assert G.newline_trips(5, G.NEWLINE_ONE_TRIP - 5) == (1, 1) and G.newline_trips(15, G.NEWLINE_ONE_TRIP + 1) == (2, 1)
    assert G.newline_trips(37, 70) == (1, 0) and G.newline_trips(35, 41) == (1, 0)
    # the lanes that go round again are the first 256: byte 83 and the byte 8 MiB behind it are the same lane's
    assert (83 // 16) % (G.NEWLINE_GROUPS * 256) == ((G.NEWLINE_ONE_TRIP + 87) // 16) % (G.NEWLINE_GROUPS * 256) == 5
    assert G.NEWLINE_TEXT // 16 - G.NEWLINE_GROUPS * 256 == 256
    # offsets from 2^32 + 5 on: the answer (a newline's offset + 1) does not fit 32 bits
    assert (G.FOUR_GIB + 5 + 1) >> 32 == 1 and G.FOUR_GIB == 4294967296


def test_the_scans_restatement_against_the_emulator(lib):
    for n in G.SCAN_SMALL:
        for kind in G.SCAN_KINDS if n <= G.TILE + 1 else ("mixed",):     # (the emulator takes a second for 64 tiles)
            v = G.scan_values(kind, n)
            want = G.scan_expected(v)
            work = np.ascontiguousarray(v if n else np.zeros(1, np.uint32))
            assert lib.sort_wave_scan(_ptr(work), ctypes.c_uint64(n), ctypes.c_uint32(G.MAX_PARTS)) == 0
            assert np.array_equal(work[:n], want), (n, kind)
    # several tiles a part with a running carry, and more than 64 parts of them, at a size the emulator walks quickly: the plan that
    # S1 + 1 has on the device with MAX_PARTS, here with 66 parts at the most
    n = 130 * G.TILE + 5
    assert G.plan(n, 66)[1:] == (2, 66)
    v = G.scan_values("mixed", n)
    want = G.scan_expected(v)
    assert lib.sort_wave_scan(_ptr(v), ctypes.c_uint64(n), ctypes.c_uint32(66)) == 0
    assert np.array_equal(v, want)


def test_the_scans_values():
    v = G.scan_values("mixed", 5000)
    assert not v[::7].any() and int(v.max()) == 8 and set(np.unique(v)) == set(range(9))
    full = G.scan_values("full", G.S1 + 1)
    assert int(full.astype(np.uint64).sum()) == (1 << 32) - 1 and np.all(full[:-1] == 2047)
    want = G.scan_expected(full)
    assert int(want[-1]) == 0xFFFFFFFF and int(want[-2]) == 2047 * G.S1
    assert np.all(np.diff(want.astype(np.int64)) > 0)                                   # (nothing wraps on the way)
    small = G.scan_values("mixed", 300)
    run, plain = 0, []
    for x in small.tolist():
        run += x
        plain.append(run & 0xFFFFFFFF)
    assert G.scan_expected(small).tolist() == plain


def test_the_keys_fields_and_their_restatement():
    for n in (1, 257, G.G1 + 1):
        tid, pos = G.key_fields(n)
        assert tid.dtype == np.int32 and pos.dtype == np.int32 and tid.min() >= 0 and pos.min() >= 0
        assert {0, G.TOP} <= set(tid[[0, -1]].tolist()) | set(pos[[0, -1]].tolist())
        keys = G.keys_expected(tid, pos)
        for k in sorted({0, 1 % n, n // 2, n - 1, min(G.G1, n - 1)}):
            assert int(keys[k]) == int(tid[k]) << 32 | int(pos[k])
    tid, pos = G.key_fields(G.G1 + 1)
    assert (int(tid[1]), int(pos[1])) == (G.TOP, G.TOP) and {int(tid[G.G1]), int(pos[G.G1])} == {0, G.TOP}


def test_the_gathers_restatement_against_plain_python():
    for n in (1, 257, 3000):
        c = G.GatherCase(n)
        assert sorted(c.perm.tolist()) == list(range(n))
        assert int((c.counts == 1000).sum()) >= 1 and (n < 7 or not c.counts[7::7][c.counts[7::7] != 1000].any())
        assert np.array_equal(c.cigar >> 4, np.repeat(np.arange(n), c.counts))
        want = c.expected()
        assert len(want["cigar"]) == len(c.cigar) and len(want["cig_off"]) == n + 1 and want["counts"][0] == 0
        assert np.array_equal(G.scan_expected(want["counts"]), want["cig_off"])
        assert np.array_equal(c.keys >> np.uint64(32), want["tid"].astype(np.uint64))
        for k in range(n):
            pos, flag, xs, ops = c.expected_slowly(k)
            a, b = int(want["cig_off"][k]), int(want["cig_off"][k + 1])
            assert (int(want["pos"][k]), int(want["flag"][k]), int(want["xs"][k]), want["cigar"][a:b].tolist()) == (pos, flag, xs, ops)
            assert all(w >> 4 == int(c.perm[k]) for w in ops)
    assert set(np.unique(G.GatherCase(3000).xs).tolist()) == {0, ord("+"), ord("-")}


def test_the_large_files_records_are_ordercases_records():
    tid, pos, flag, op = G.decode_fields(2000)
    raw = G.bam_records(tid, pos, flag, op)
    assert raw == b"".join(O.record(int(t), int(p), int(f), 60, [int(o)]) for t, p, f, o in zip(tid, pos, flag, op))
    assert set(tid.tolist()) == {0, 1, 2} and pos.min() >= 1 and pos.max() <= 4096 and np.array_equal(op >> 4, 1 + np.arange(2000) % 1000)
    # the expectation is ordercases' own: numpy's stable sort of the placed records, reference by reference
    recs = [(int(t), int(p), int(f), 60, [int(o)], b"") for t, p, f, o in zip(tid, pos, flag, op)]
    want = O.expected(recs, 3)
    for t in range(3):
        p, f, off, cig = G.decode_expected(tid, pos, flag, op, t)
        rs = want[t][0]
        assert np.array_equal(p, rs.pos) and np.array_equal(f, rs.flag) and np.array_equal(off, rs.cig_off) and np.array_equal(cig, rs.cigar)
        assert len(np.unique(p)) < len(p)           # (ties: the order is the stable sort's to decide)
