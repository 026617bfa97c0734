"""CPU checks of classcases.py (test_gpu_class_limits.py runs the cases on the GPU): every read lands in the run the case declares,
every limit value occurs in every spelling, limitcases.read_class agrees where it claims to know, the host build of the per-read
core counts what the oracle counts -- and the cases can fail: the oracle's counters change when any one packed field is decoded
wrongly.  No GPU."""
import numpy as np
import pytest

import classcases as K
import limitcases as L
from hostsim import sim
from spliser_amd import native


def _oracle(oracle_lib, t, rs, stranded, combine=0):
    return oracle_lib.check_bam(t.pos, t.strand, t.part_off, t.part_pos, t.comp_off, t.comp_pos, rs.pos, rs.flag, rs.cig_off, rs.cigar,
                                stranded, combine)


@pytest.mark.parametrize("name", K.NAMES)
def test_the_host_packer_puts_every_read_in_its_declared_run(name):
    """The packed bytes, unpacked again: every chunk's runs hold the reads the case declares for them, in file order, with the
    lengths the reads have (test_pack_host.unpack reads the fields back with the header's layout)."""
    import test_pack_host as T
    case = K.case(name)
    sets = [(case.reads, case.meta["runs"], case.meta["records"])]
    if name == "top":
        bad = case.meta["bad_records"]
        sets.append((L.reads_from(bad), np.array([K.declared_run(*r) for r in bad]), bad))
    for rs, runs, recs in sets:
        assert rs.n == len(runs) <= K.MAX_READS
        desc, rec, wide = native.pack_host(native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar), threads=2)
        got = T.unpack(desc, rec, wide)
        for c, chunk_runs in enumerate(got):
            lo, hi = c * T.CHUNK, min(rs.n, (c + 1) * T.CHUNK)
            for run in range(4):
                want = [(p, f, T.classify(p, f, [(ln << 4) | code for ln, code in ops])[1]) for (f, p, ops), r in zip(recs[lo:hi], runs[lo:hi])
                        if r == run]
                assert chunk_runs[run] == want, (name, c, run)
    if name == "top":       # the twins are refused by every class: they reach the general path, which reports them
        assert all(K.declared_run(*r) == 3 for r in case.meta["twins"])
        assert all(p + sum(K.consuming_lens(ops)) == K.COORD_MAX + 1 for _, p, ops in case.meta["twins"])
        good = [r for r in case.meta["records"] if len(K.consuming_lens(r[2])) in (3, 5) and r[1] + sum(K.consuming_lens(r[2])) == K.COORD_MAX]
        assert len(good) >= 4 * 7 * 4 and all((K.declared_run(*r) == 3) == (len(r[2]) > K.SCAN_OPS) for r in good)
        assert case.segments[0][1] == K.TOP_SHIFT > (1 << 31) - (1 << 17) and case.table.pos[-1] == K.COORD_MAX


@pytest.mark.parametrize("name", ["simple", "once_spliced", "twice_spliced", "queued", "top"])
def test_every_limit_value_occurs_in_every_spelling(name):
    """From the ops: the reference-consuming lengths say which value a read carries, the other ops which classifier meets it."""
    case = K.case(name)
    seen = {}
    for (f, p, ops), run in zip(case.meta["records"], case.meta["runs"]):
        if f & 4:
            continue
        lens = K.consuming_lens(ops)
        for label, pred in K.REQUIRED[name]:
            if K.shape_of(ops) and pred(lens):
                seen.setdefault((label, K.spelling_of(ops)), set()).add(int(run))
    for label, _ in K.REQUIRED[name]:
        for sp in K.SPELLINGS:
            assert (label, sp) in seen, (name, label, sp)
            # nine ops are WIDE as they stand; every other spelling is packed by its reference-consuming ops
            if sp == "wide9":
                assert seen[(label, sp)] == {3}, (label, sp)
            else:
                assert seen[(label, sp)] == seen[(label, "plain")], (label, sp)
    # the values on the packed side of a limit are packed, those beyond it are not
    plain = {label: runs for (label, sp), runs in seen.items() if sp == "plain"}
    if name == "simple":
        assert [plain["len=%d" % v] for v in K.LIMITS] == [{0}, {0}, {3}, {3}, {3}]
    if name in ("once_spliced", "queued"):
        assert [plain["mnm a=%d" % v] for v in K.LIMITS] == [{1}, {1}, {3}, {3}, {3}]
        assert [plain["mnm b=%d" % v] for v in K.LONG_B] == [{1}, {1}, {1}]          # b is a full word: the read stays MNM
    if name == "once_spliced":
        assert plain["mnm d=1"] == plain["mnm d=%d" % K.BIG_D] == {1}
    if name in ("twice_spliced", "queued"):
        for k in "abc":
            assert [plain["m2 %s=%d" % (k, v)] for v in K.EDGE16] == [{2}, {2}, {2}, {3}], k
    if name == "twice_spliced":
        assert plain["a=b=c=65535"] == plain["d1=d2=2^28-1"] == {2}


def test_simple_limit_reads_start_inside_the_window_and_leave_it():
    """Every chunk, of either size: a simple limit read's range begins inside the chunk's LDS window (the smallest one, the stranded
    fused pass's) and ends more than the largest window's entries behind the window's base."""
    case = K.case("simple")
    dpos = case.table.dpos()
    recs = case.meta["records"]
    n_seen = 0
    for chunk in (L.CHUNK, L.CHUNK_BIG):
        for c0 in range(0, len(recs), chunk):
            wbase = L.window_base(case.table, recs[c0][1])
            for f, p, ops in recs[c0:c0 + chunk]:
                lens = K.consuming_lens(ops)
                if len(lens) != 1 or lens[0] < K.LIMITS[0]:
                    continue
                lo = int(np.searchsorted(dpos, p - 1, side="right"))
                ub = int(np.searchsorted(dpos, p + lens[0] - 1, side="left"))
                assert wbase <= lo < wbase + L.WIN_STRANDED_FUSED and ub > wbase + L.WIN, (chunk, c0, p, lens)
                n_seen += 1
    assert n_seen > 1000


def test_junction_ends_are_rows_and_rivals_are_what_the_cases_say():
    t = K.table()
    rows = set(t.pos.tolist())
    assert 3000 <= t.n <= 3700 and len(set(t.strand.tolist())) == 2
    for name in ("once_spliced", "twice_spliced", "queued"):
        for f, p, ops in K.distinct(K.case(name).meta["records"]):
            if K.shape_of(ops) in ("ANA", "ANANA"):
                lens = K.consuming_lens(ops)
                for l, r in K.junctions_of(p, lens):
                    assert l in rows and r in rows, (name, p, lens)
    for (kl, kr), riv in K.RIVALS:
        assert sorted(int(t.pos[x]) for x in t.rivals(K.gpos(kl), K.gpos(kr))) == [K.gpos(k) for k in riv]
    counts = sorted(len(r) for _, r in K.RIVALS)
    assert counts[-1] == L.RIV_TWICE + 1 and L.RIV_ONCE + 1 in counts and counts[0] <= L.RIV_ONCE
    q = K.case("queued")
    assert q.meta["n_listed"] >= int(np.count_nonzero(q.reads.flag & 4)) + 400
    runs = q.meta["runs"][(q.reads.flag & 4) == 0]
    assert all(np.count_nonzero(runs == r) > 100 for r in (1, 2))
    top = K.case("top").table
    assert top.pos[-1] == K.COORD_MAX and len(top.rivals(*K.junctions_of(*K.top_shapes()[2])[0])) == 1


def test_long_reads_are_what_they_claim():
    case = K.case("long_reads")
    recs = case.meta["records"]
    assert len(recs) == L.CHUNK + 100 and [r[1] for r in recs] == sorted(r[1] for r in recs)
    rows = set(case.table.pos.tolist())
    n_ops = [len(ops) for _, _, ops in recs]
    assert min(n_ops) >= 20 and max(n_ops) <= 400 and max(n_ops) > 380
    blocks = [ln for _, _, ops in recs for ln, c in ops if c == L.M]
    assert min(blocks) == 1 and max(blocks) == 3000
    on_rows = total = 0
    for f, p, ops in recs:
        n_n = sum(c == L.N for _, c in ops)
        assert 2 <= n_n <= 15 and all(1 <= ln <= 5 for ln, c in ops if c in (L.I, L.D))
        cur = p
        for ln, c in ops:
            if c == L.N:
                total += 2
                on_rows += (cur - 1 in rows) + (cur + ln - 1 in rows)
            cur += ln if c in K.CONSUMING else 0
    assert on_rows > 0.9 * total                      # (a read that runs past the last row ends its junctions there)
    assert any(ops[0][1] == L.S for _, _, ops in recs) and any(ops[-1][1] == L.S for _, _, ops in recs)
    assert set(case.meta["runs"].tolist()) == {3}


@pytest.mark.parametrize("name", K.NAMES)
def test_read_class_agrees_with_the_declared_run(name):
    """limitcases.read_class knows CIGARs of M, N, = and X ops of reads inside the coordinate space."""
    case = K.case(name)
    n = 0
    for (f, p, ops), run in zip(case.meta["records"], case.meta["runs"]):
        if all(c in (L.M, L.N, L.EQ, L.X) for _, c in ops) and p >= 0 and p + sum(K.consuming_lens(ops)) <= K.COORD_MAX:
            assert L.read_class(ops, f) == run, (name, f, p, ops)
            n += 1
    assert n > 0 or name == "long_reads"


@pytest.mark.parametrize("name", K.NAMES)
def test_the_host_core_counts_the_distinct_reads_like_the_oracle(name, oracle_lib):
    case = K.case(name)
    recs = K.distinct(case.meta["records"])
    rs = L.reads_from(recs)
    for stranded, combine in ([(0, 0), (1, 1)] if name == "long_reads" else case.modes):     # (long_reads: the slow ones on the host)
        if True:
            want = _oracle(oracle_lib, case.table, rs, stranded, combine)
            got = sim.count(case.table, rs, stranded, combine)
            for w, g in zip(want, got):
                assert np.array_equal(w, g), (name, stranded, combine)
            assert int(want[0].sum()) > 0 and int(want[1].sum()) > 0


# ---- the cases can fail ---------------------------------------------------------------------------------------------------------

def _family_of(field):
    return [fam for fam, fields in K.FAMILY_FIELDS.items() if field in fields][0]


@pytest.mark.parametrize("field,damage", K.DAMAGES)
def test_a_damaged_field_changes_the_oracles_counters(field, damage, oracle_lib):
    """One packed field decoded wrongly, one damage at a time, on the distinct reads of the field's own family and of `queued`: the
    oracle counts something else in at least one row, unstranded and stranded."""
    for name in (_family_of(field), "queued"):
        case = K.case(name)
        recs = K.distinct(case.meta["records"])
        bad, changed = K.damaged(recs, field, damage)
        assert changed > 0, (name, field, damage)
        for stranded in (0, 1):
            true = _oracle(oracle_lib, case.table, L.reads_from(recs), stranded)
            wrong = _oracle(oracle_lib, case.table, L.reads_from(bad), stranded)
            assert any(not np.array_equal(a, b) for a, b in zip(true[:2], wrong[:2])), (name, field, damage, stranded)


@pytest.mark.parametrize("field", ["mnm_a", "mnm_b", "m2_a", "m2_b", "m2_c"])
def test_a_damaged_field_shows_at_the_top_of_the_coordinate_space(field, oracle_lib):
    case = K.case("top")
    recs = K.distinct(case.meta["records"])
    bad, changed = K.damaged(recs, field, "&0x7fff")
    assert changed > 0
    for stranded in (0, 1):
        true = _oracle(oracle_lib, case.table, L.reads_from(recs), stranded)
        wrong = _oracle(oracle_lib, case.table, L.reads_from(bad), stranded)
        assert any(not np.array_equal(a, b) for a, b in zip(true[:2], wrong[:2])), (field, stranded)


def test_the_damages_cover_every_field():
    for field in K.FIELDS:
        have = {d for f, d in K.DAMAGES if f == field}
        assert {"&0xfff", "&0x7fff", "wrap65536"} <= have
    assert ("mnm_b", "&0xffff") in K.DAMAGES and ("m2_b", "swap_bc") in K.DAMAGES
