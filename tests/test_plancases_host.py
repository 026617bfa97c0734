"""CPU checks that the worlds of plancases.py reach what they are named for (test_gpu_process_plans.py runs them through ``process``
on the GPU): a change to a world, to ``shard.pack`` or to the room the first plan leaves that made a world miss its route through
``process_sites`` would otherwise leave its GPU test passing without testing anything."""
import ctypes

import numpy as np
import pytest

import plancases as P
from spliser_amd import native, samio, shard


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = tmp_path_factory.mktemp("plans")
    out = {}
    for name in P.NAMES:
        w = P.world(name)
        prefix = str(root / name)
        out[name] = (w, prefix, P.write_files(w, prefix), P.table_of(prefix + ".bed", None))
    return out


def _where(shards, chrom):
    for k, sh in enumerate(shards):
        if chrom in sh.chroms:
            j = sh.chroms.index(chrom)
            return k, j, sh.offsets[j], sh.limits[j]
    raise KeyError(chrom)


@pytest.mark.parametrize("name", P.NAMES)
def test_the_plans_have_the_shape_the_world_is_named_for(files, name):
    w, _, _, table = files[name]
    first, exact = P.plans(w, table)
    assert [sh.chroms for sh in first] == P.SHAPES[name][0]
    assert [sh.chroms for sh in exact] == P.SHAPES[name][1]
    for sh in first + exact:      # every shard stays inside the coordinate space, whatever the header said
        assert max(off + lim for off, lim in zip(sh.offsets, sh.limits)) <= shard.COORD_MAX
    for ref, rs in zip(w.refs, w.sets):
        _, _, _, limit = _where(first, ref.name)
        _, _, _, room = _where(exact, ref.name)
        assert rs.max_end <= room                                     # the exact plan has room for every read ...
        assert (rs.max_end > limit) == (ref.name == w.understated)    # ... the first one for all but the understated reference's
        if ref.n:
            assert rs.n == ref.n + len(ref.spill) and int(rs.pos.min()) < 1100 and rs.max_end >= ref.end
            assert ref.end + 1000 < ref.ln or ref.name == w.understated      # (an honest header: the reads end below LN)


def test_the_understated_reference_is_where_its_world_says(files):
    # last: alone with the 5e8 reference (and the two without reads) in the third shard, so that two shards are counted or laid out before it
    w, _, _, table = files["overhang_last"]
    first, _ = P.plans(w, table)
    assert _where(first, "c6")[:2] == (2, 1) and _where(first, "c5")[:2] == (2, 0)
    assert _where(first, "c6")[3] == 3_000_000 - 200 < w.sets[w.names.index("c6")].max_end == 3_000_000     # its slot ends at its last site
    # first: in the first shard, before anything else
    w, _, _, table = files["overhang_first"]
    first, exact = P.plans(w, table)
    assert _where(first, "c1")[:2] == (0, 0) and _where(first, "c1")[3] < w.sets[0].max_end
    assert len(first) == 2 and len(exact) == 1       # ... and the second plan's shards are composed differently from the first's
    # cut_overhang is overhang_last's header and reads
    assert files["cut_overhang"][0].lengths == files["overhang_last"][0].lengths
    assert all(samio_equal(a, b) for a, b in zip(files["cut_overhang"][0].sets, files["overhang_last"][0].sets))


def samio_equal(a, b):
    return a.n == b.n and np.array_equal(a.pos, b.pos) and np.array_equal(a.flag, b.flag) and np.array_equal(a.cigar, b.cigar)


def test_overhang_middle_spills_onto_the_next_references_sites_and_stays_in_the_space(files):
    """Were the limit missed, c2's last reads would be counted on c3's first locus: a wrong count, not a coordinate out of range."""
    w, _, _, table = files["overhang_middle"]
    first, _ = P.plans(w, table)
    (k1, j1, _, _), (k2, j2, off2, lim2), (k3, j3, off3, _) = (_where(first, c) for c in ("c1", "c2", "c3"))
    assert k1 == k2 == k3 == 0 and (j1, j2, j3) == (0, 1, 2)
    rs = w.sets[1]
    arr3 = table.chrom_arrays("c3")
    assert rs.max_end > lim2 + shard.GAP                               # beyond the gap: into c3's slot
    assert off2 + rs.max_end < off3 + int(arr3.pos.max())              # ... but not beyond c3's sites,
    assert off2 + rs.max_end < shard.COORD_MAX                         # ... let alone the coordinate space
    # the spilled reads, seen in c3's coordinates, lie across sites of c3's first locus (one-op reads: they would add to beta1)
    spilled = rs.pos[rs.pos > lim2 + shard.GAP].astype(np.int64) + off2 - off3
    assert len(spilled) == len(w.refs[1].spill)
    hit = set()
    for p in spilled.tolist():
        hit.update(int(s) for s in arr3.pos if p <= s and p + 100 > s + 1)
    assert len(hit) >= 5
    # and they make no site of c2's own: its slot ends at the last site of its second locus
    assert lim2 == int(table.chrom_arrays("c2").pos.max()) == w.refs[1].end - P.TAIL_END + P.LAST_SITE


@pytest.mark.parametrize("stranded", [None, "fr"])
@pytest.mark.parametrize("name", P.NAMES)
def test_every_reference_with_reads_has_every_kind_of_count(files, oracle_lib, name, stranded):
    """A world whose reads hit nothing would pass any plan."""
    w, prefix, _, _ = files[name]
    table = P.table_of(prefix + ".bed", stranded)
    assert list(table.chrom_index)[0] == "ghost" and list(table.chrom_index)[1:] == w.names
    for chrom in table.chrom_index:
        arr = table.chrom_arrays(chrom)
        rd = w.sets[w.names.index(chrom)] if chrom in w.names else samio.ReadSet.empty()
        res, dbl = P.oracle_counts(oracle_lib, arr, rd, stranded, bool(stranded))
        assert arr.n and int(arr.alpha.sum()) > 0
        if rd.n:
            assert set(np.unique(rd.flag).tolist()) == {0, 16, 83, 99, 147, 163}
            assert sorted(set(np.diff(rd.cig_off.astype(np.int64)).tolist())) == [1, 3, 5]
            for half in (arr.pos < 3000, arr.pos >= 3000):      # both loci
                assert int(res["beta1"][half].sum()) > 0 and int(res["beta2_simple"][half].sum()) > 0
                assert np.count_nonzero(res["sse"][half]) and np.count_nonzero(res["beta2_weighted"][half])
            assert int(dbl.sum()) > 0 and np.count_nonzero(dbl) >= 4
        else:
            assert int(res["beta1"].sum()) == 0 and not np.any(dbl)
    text = P.oracle_tsv(oracle_lib, prefix + ".bed", w.names, w.sets, stranded, bool(stranded))
    assert text.count("\n") == 1 + sum(table.chrom_arrays(c).n for c in table.chrom_index)


def _shares(path, n_shares):
    """What each of ``n_shares`` shares of the file holds, by the host's walk -> [records per reference]."""
    native.build()
    bam = native.BamFile(path, defer=True)
    try:
        n = ctypes.c_int(0)
        native._check(native.lib().spl_bam_share_plan(bam._h, ctypes.c_int(n_shares), ctypes.byref(n)))
        assert n.value == n_shares
        return [bam.share_count_host(k)[:-1] for k in range(n_shares)]
    finally:
        bam.close()


@pytest.mark.parametrize("name,n_shares", [("cut", 3), ("cut", 5), ("cut_overhang", 3), ("cut_overhang", 5), ("cut_overhang_late", 3), ("cut_three_shards", 3), ("declined", 3)])
def test_the_shares_cut_chromosomes(files, name, n_shares):
    w, prefix, _, table = files[name]
    held = np.array(_shares(prefix + ".bam", n_shares))
    assert held.sum(axis=0).tolist() == [rs.n for rs in w.sets]        # every read in exactly one share
    assert np.all(held.sum(axis=1) > 0)                                # no share without reads
    cut = [c for c, col in zip(w.names, held.T) if np.count_nonzero(col) > 1]
    assert len(cut) >= 2, held
    if name in ("cut", "declined"):
        return
    # The last of three shares holds the rest of c2 and every reference behind it, in two shards by overhang_last's header: the
    # understated reference is in the second, so the context plans again before it has counted anything.  With a fifth reference that leaves
    # no room for it beside c4 and c5 (cut_overhang_late) it is in the third: the first shard, with the piece of c2, is counted and handed over, then the
    # context plans again.  Of five shares the last holds a piece of c3 and what is behind it.
    mine = [c for c, n in zip(w.names, held[-1]) if n] + ["empty"]
    assert mine == (["c2", "c3", "c4", "c5", "c6", "empty"] if n_shares == 3 else ["c3", "c4", "c5", "c6", "empty"])
    assert mine[0] in cut
    first, _ = P.plans(w, table, mine)
    if name == "cut_overhang_late":
        assert [sh.chroms for sh in first] == [["c2", "c3"], ["c4", "c5"], ["c6", "empty"]]
    elif n_shares == 3:
        assert [sh.chroms for sh in first] == [["c2", "c3"], ["c4", "c5", "c6", "empty"]]
    else:
        assert [sh.chroms for sh in first] == [["c3", "c4"], ["c5", "c6", "empty"]]


def test_the_declined_world_is_cuts_reads_with_parked_cigars(files):
    w, prefix, recs, _ = files["declined"]
    cut = files["cut"][0]
    assert w.lengths == cut.lengths and all(samio_equal(a, b) for a, b in zip(w.sets, cut.sets))
    parked = [r for r in recs if r[5][:4] == b"CGBI"]
    assert len(parked) > 100 and all(len(r[4]) == 2 and int(r[4][0]) == 4 for r in parked)
    # the host decoder reads them as the reads they are
    native.build()
    bam = native.BamFile(prefix + ".bam")
    try:
        for c, rs in zip(w.names, w.sets):
            got = bam.reads(c)
            assert got.n == rs.n and (rs.n == 0 or samio_equal(got, rs))
    finally:
        bam.close()


def test_the_unsorted_world_has_half_of_c1_behind_the_last_reference(files):
    w, prefix, recs, _ = files["unsorted_three_shards"]
    tids = [r[0] for r in recs]
    n1 = w.sets[0].n
    assert tids[:n1 // 2] == [0] * (n1 // 2) and tids[-(n1 - n1 // 2):] == [0] * (n1 - n1 // 2) and 0 not in tids[n1 // 2:-(n1 - n1 // 2)]
    assert recs[-1][1] > 900_000_000 > recs[n1 // 2 - 1][1]             # the second locus is in the late half
    native.build()
    bam = native.BamFile(prefix + ".bam", stream=True)
    try:
        assert bam.wait_all() is False
        assert samio_equal(bam.reads("c1"), w.sets[0])
    finally:
        bam.close()
