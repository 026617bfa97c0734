"""CPU checks that the cases of junctioncases.py reach the limits they are built for (test_gpu_junction_limits.py runs them on the
GPU against oracle.junction_table): a case that drifted off its limit would leave its GPU test passing without testing it."""
import junctioncases as J


def test_the_constants_come_from_the_kernel_sources():
    assert J.S_OPS_ROW == 5                                  # a lane rebuilds at most M N M N M
    assert J.HASH == 0x9E3779B97F4A7C15
    assert J.MIN_SLOTS & (J.MIN_SLOTS - 1) == 0 and J.MIN_SLOTS >= 64
    assert J.CHUNK_BIG == 2 * J.CHUNK
    assert J.NOPS_SAT < (1 << 16) and J.COORD_MAX < (1 << 31)


def test_slot_arithmetic():
    assert J.n_slots(0) == J.n_slots(J.MIN_SLOTS) == J.MIN_SLOTS
    assert J.n_slots(J.MIN_SLOTS + 1) == 2 * J.MIN_SLOTS
    assert J.n_slots(233709) == 1 << 18
    k = J.key_of(5, 9, True)
    assert k == (5 << 32) | (9 << 1) | 1 and J.key_of(5, 9) == k - 1
    assert J.key_of(-1, 9) >> 32 == 0xffffffff
    # linear probing: a run of keys with one home fills the slots after it, and wraps
    keys = [J.key_of(l, r) for l, r in J.hash_case().meta["hot"]]
    got = J.place(keys, J.MIN_SLOTS)
    assert sorted(got.values()) == sorted(((J.MIN_SLOTS - 10 + i) & (J.MIN_SLOTS - 1)) for i in range(len(keys)))


def test_every_record_class_carries_junctions():
    case = J.record_classes_case()
    seen = set()
    for rec in case.recs:
        run, wide = J.packed_run(rec)
        if J.junctions_of(rec) or rec[0] & 4:
            seen.add((run, wide, bool(rec[0] & 4)))
    assert {(1, False, False), (2, False, False), (3, False, False), (3, True, False), (3, False, True), (3, True, True)} <= seen
    assert any(J.packed_run(r) == (0, False) for r in case.recs)                     # SIMPLE: no junction
    # the class limits: MNM's first block < 2^16 (one past: OTHER), M2's blocks < 2^16 in the host packer
    by_first = {(len(r[2]), r[2][0][0]): J.packed_run(r)[0] for r in case.recs if r[2] and r[2][0][1] == J.M}
    assert by_first[(3, (1 << 16) - 1)] == 1 and by_first[(3, 1 << 16)] == 3
    assert by_first[(5, 4095)] == by_first[(5, 4096)] == by_first[(5, 65535)] == 2 and by_first[(5, 65536)] == 3
    # a read of more ops than the packed count holds; reads with I / S / H / P / D / = / X around N ops; '*' CIGARs
    assert case.meta["n_ops_long"] > J.NOPS_SAT
    codes = {c for _, _, ops in case.recs if any(c == J.N for _, c in ops) for _, c in ops}
    assert {J.I, J.S, J.H, J.P, J.D, J.EQ, J.X} <= codes
    assert sum(1 for r in case.recs if not r[2]) >= 2
    # the OTHER-narrow records keep their three ops in the record: at most the row a lane rebuilds
    assert all(len([o for o in r[2] if o[1] in (J.M, J.D, J.N, J.EQ, J.X)]) <= J.S_OPS_ROW for r in case.recs if J.packed_run(r) == (3, False))


def test_filter_boundaries_sit_on_the_reads_values():
    case = J.filter_boundaries_case()
    A1, A2 = case.meta["anchors"]
    Dn = case.meta["intron"]
    js = [j for r in case.recs for j in J.junctions_of(r)]
    anchors = {j[3] for j in js} | {j[4] for j in js}
    introns = {j[2] for j in js}
    assert {0, A1, A2} <= anchors and {0, Dn - 1, Dn, Dn + 1} <= introns
    filt = set(case.filters)
    for a in (A1, A2):
        assert {(a - 1, 0, 0), (a, 0, 0), (a + 1, 0, 0)} <= filt
    assert {(0, Dn - 1, 0), (0, Dn, 0), (0, Dn + 1, 0), (0, 0, Dn - 1), (0, 0, Dn), (0, 0, Dn + 1), (0, 1, 0), (0, 0, 0)} <= filt
    # a read whose first N op passes -m 70 and whose next one fails, and one whose failed N op ends the next one's left anchor
    assert any([J.passes(j, 0, 70, 0) for j in J.junctions_of(r)][:2] == [True, False] for r in case.recs)
    assert any([(J.passes(j, 0, 70, 0), j[3]) for j in J.junctions_of(r)] == [(False, 20), (True, 3)] for r in case.recs)
    assert {-1, 0} <= {j[0] for j in js}                                # N ops at POS 0 and 1
    # every setting keeps some junctions and drops others
    for a, m, mx in case.filters:
        keep = [J.passes(j, a, m, mx) for j in js]
        assert any(keep) and (not all(keep) or (a, m, mx) == (0, 0, 0)), (a, m, mx)


def test_wave_merge_maxima_come_from_non_leader_lanes():
    case = J.wave_merge_case()
    L, R = case.meta["junction"]
    (lane_l, max_l), (lane_r, max_r) = case.meta["max_left"], case.meta["max_right"]
    assert {J.packed_run(r) for r in case.recs} == {(3, True)}         # one class: slots are the reads' places at either chunk size
    for chunk in (J.CHUNK, J.CHUNK_BIG):
        for stranded in (0, 1, 2):
            groups = [g for g in J.wave_groups(case.recs, chunk, stranded)
                      if g["key"] >> 32 == L and (g["key"] & 0xffffffff) >> 1 == R]
            rounds = {}
            for g in groups:
                rounds.setdefault(g["wave"], set()).add(g["round"])
            assert all(len(q) >= 2 for q in rounds.values()) and len(rounds) == 2   # both waves reach J in two rounds
            top = [g for g in groups if lane_l in g["lanes"] and lane_r in g["lanes"] and g["wave"] == (0, 0)]
            assert len(top) == 1
            g = top[0]
            assert g["leader"] not in (lane_l, lane_r) and lane_l != lane_r
            assert g["lanes"][g["leader"]][0] < max_l and g["lanes"][g["leader"]][1] < max_r
    # the maxima are unique over the whole set: only those two lanes can give them
    js = [(j, i) for i, r in enumerate(case.recs) for j in J.junctions_of(r) if j[:2] == (L, R)]
    assert [i for j, i in js if j[3] >= max_l] == [lane_l] and [i for j, i in js if j[4] >= max_r] == [lane_r]


def test_many_chunks_count_past_16_bits():
    case = J.many_chunks_case()
    L, R = case.meta["junction"]
    for stranded in (0, 1, 2):
        row = [w for w in case.want(stranded, 0, 0, 0) if w[:2] == (L, R)]
        assert len(row) == 1 and row[0][3] > 65535 and row[0][4:] == (case.meta["max_left"], case.meta["max_right"])
    idx = [(i, j) for i, r in enumerate(case.recs) for j in J.junctions_of(r) if j[:2] == (L, R)]
    left = [i for i, j in idx if j[3] == case.meta["max_left"]]
    right = [i for i, j in idx if j[4] == case.meta["max_right"]]
    assert len(left) == len(right) == 1
    for chunk in (J.CHUNK, J.CHUNK_BIG):
        chunks = {i // chunk for i, _ in idx}
        assert len(chunks) > 3 * J.CHUNK_BIG // chunk
        assert left[0] // chunk not in (0, right[0] // chunk) and right[0] // chunk != max(chunks)


def test_hash_keys_collide_and_wrap():
    case = J.hash_case()
    mask = case.meta["mask"]
    n_ops = int(case.reads.cig_off[-1])
    assert J.n_slots(n_ops) == J.MIN_SLOTS == mask + 1
    hot = [J.key_of(l, r) for l, r in case.meta["hot"]]
    assert len(set(hot)) >= 40 and {J.home(k, mask) for k in hot} == {mask - 9}
    keys = sorted({J.key_of(j[0], j[1]) for r in case.recs for j in J.junctions_of(r)})
    where = J.place(keys, mask + 1)
    used = set(where.values())
    assert mask in used and 0 in used                                     # the run passes the last slot and goes on at 0
    assert all(J.home(J.key_of(l, r), mask) == 1 for l, r in case.meta["low"])
    assert any(where[J.key_of(l, r)] != 1 for l, r in case.meta["low"])    # ... and meets keys whose home is there
    # the same (l, r) on both strands, paired and unpaired
    Lb, Rb = case.meta["both"]
    flags = {r[0] for r in case.recs if any(j[:2] == (Lb, Rb) for j in J.junctions_of(r))}
    assert flags == {0, 16, 99, 147, 83, 163}
    for stranded in (1, 2):
        assert {w[2] for w in case.want(stranded, 0, 0, 0) if w[:2] == (Lb, Rb)} == {ord("+"), ord("-")}
    assert [w[2] for w in case.want(0, 0, 0, 0) if w[:2] == (Lb, Rb)] == [ord("?")]


def test_coordinates_reach_the_top_of_the_shard_space():
    case = J.coordinates_case()
    js = [j for r in case.recs for j in J.junctions_of(r)]
    assert any(j[0] == (1 << 30) - 1 for j in js) and any(j[1] == (1 << 30) - 1 for j in js)
    assert any(j[1] >= 1 << 30 for j in js)
    ends = [p + sum(ln for ln, c in ops if c in (J.M, J.D, J.N, J.EQ, J.X)) for _, p, ops in case.recs]
    assert max(ends) == J.COORD_MAX and ends.count(J.COORD_MAX) >= 3
    assert max(j[1] for j in js) == J.COORD_MAX - 1
    bad = J.records(J.beyond_coord_max())
    assert max(p + sum(ln for ln, c in ops if c in (J.M, J.N)) for _, p, ops in bad) == J.COORD_MAX + 1


def test_shifted_and_empty_cases():
    case = J.shifted_case()
    assert len(case.segments) == 3 and all(shift for _, shift in case.segments)
    assert min(r[1] for r in case.recs) >= min(shift for _, shift in case.segments)
    assert J.case("empty").reads.n == 0
    only = J.case("only_unmapped")
    assert only.reads.n and all(r[0] & 4 for r in only.recs) and only.want(0, 0, 0, 0) == []
