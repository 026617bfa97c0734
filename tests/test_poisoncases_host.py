"""CPU checks of poisoncases.py (test_gpu_poisoned_memory.py runs its list on poisoned and on reused device memory): the list builds
twice to identical inputs, its names are unique and ``--list`` prints them without a GPU, every case's yardstick is non-trivial
-- what that means is stated per case, in the case's ``nontrivial`` --, and the comparator rejects a result with one counter, one run
boundary, one mate word or one byte of a file changed, case by case: a comparator that cannot fail would let the whole GPU module
prove nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest

import poisoncases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_are_unique_and_the_list_covers_every_path():
    assert len(set(P.NAMES)) == len(P.NAMES)
    for prefix, n in (("count_", 8), ("decode_", 2), ("text_", 7), ("text_windows_", 4), ("one_set_", 2), ("junctions_", 3), ("end_to_end_", 3), ("genome_", 2),
                      ("motif_", 1), ("lanes_", 1)):
        assert sum(1 for name in P.NAMES if name.startswith(prefix)) == n, prefix
    assert len(P.NAMES) == 29
    assert all(name.replace("_", "").isalnum() for name in P.NAMES)          # (they are file names)


def test_list_prints_the_names_without_a_gpu():
    """In a fresh interpreter that cannot see a device: the names come out, and the library is not even loaded."""
    code = ("import sys; sys.argv = ['poisoncases.py', '--list']; sys.path.insert(0, %r); import poisoncases as P; rc = P.main(); "
            "from spliser_amd import native; assert native._lib is None; sys.exit(rc)" % os.path.join(ROOT, "tests"))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.split() == P.NAMES
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "poisoncases.py"), "--list"], cwd=ROOT, env=env, stdout=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == P.NAMES


@pytest.mark.parametrize("name", P.NAMES)
def test_the_list_builds_twice_to_identical_inputs(name, tmp_path):
    a = P.case(name).build(str(tmp_path / "a"))
    b = P.case(name).build(str(tmp_path / "b"))
    assert P.fingerprint(a) == P.fingerprint(b) == P.fingerprint(P.inputs_of(name))
    if a:
        assert P.fingerprint(a) != P.fingerprint({})


def test_a_fingerprint_sees_one_changed_word_and_one_changed_byte_of_a_file(tmp_path):
    inp = P.case("decode_shuffled_all_switches").build(str(tmp_path / "d"))
    before = P.fingerprint(inp)
    with open(inp["shuffled_path"], "r+b") as fh:
        fh.seek(1000)
        byte = fh.read(1)
        fh.seek(1000)
        fh.write(bytes([byte[0] ^ 1]))
    assert P.fingerprint(inp) != before
    inp = P.case("count_scan_%d" % (P.L.SCAN_BLOCK + 1)).build(None)
    before = P.fingerprint(inp)
    inp["case"].reads.pos[7] += 1
    assert P.fingerprint(inp) != before


@pytest.mark.parametrize("name", P.NAMES)
def test_every_yardstick_is_non_trivial(name):
    want = P.want_of(name)
    assert want and all(isinstance(v, np.ndarray) for v in want.values())
    assert sum(v.size for v in want.values()) > 0 and any(int(np.count_nonzero(v)) for v in want.values())
    P.case(name).nontrivial(P.inputs_of(name), want)


def _changed(a):
    """``a`` with one entry changed (the middle one), or one entry more where it has none."""
    a = np.array(a)
    if a.size == 0:
        return np.zeros((1,) + a.shape[1:], a.dtype)
    flat = a.reshape(-1)
    k = flat.shape[0] // 2
    if a.dtype.kind == "f":
        flat[k] = 1.0 if flat[k] != flat[k] else np.nextafter(flat[k], np.inf) if np.isfinite(flat[k]) else 0.0
    else:
        flat[k] ^= 1
    return a


@pytest.mark.parametrize("name", P.NAMES)
def test_the_comparator_rejects_one_changed_entry_of_every_result(name):
    want = P.want_of(name)
    assert P.mismatches(want, want) == []
    assert P.mismatches({k: v.copy() for k, v in want.items()}, want) == []
    for key in want:
        got = dict(want)
        got[key] = _changed(want[key])
        bad = P.mismatches(got, want)
        assert len(bad) == 1 and bad[0].startswith(key + ":"), (name, key, bad)
        got = dict(want)
        del got[key]
        assert P.mismatches(got, want) == ["%s: missing" % key]
    extra = dict(want, one_more=np.zeros(1, np.int64))
    assert P.mismatches(extra, want) == ["one_more: not expected"]


def test_the_comparator_on_the_kinds_the_issue_names():
    """One counter, one run boundary, one mate word, one byte of a file, one word of an SSE, one base code, one counter of the motif
    tally, one row of a BED -- and what is equal stays equal through the file the driver writes: NaN, uint64 name keys, integers of
    any width."""
    w = P.want_of("one_set_every_consumer")
    for key in ("gene_counts", "coverage_start", "mate", "strand_tally", "junctions", "record_bytes_after_every_call"):
        got = dict(w)
        got[key] = w[key].copy()
        got[key].reshape(-1)[got[key].size // 3] += 1
        assert [b.split(":")[0] for b in P.mismatches(got, w)] == [key]
    shorter = dict(w, coverage_end=w["coverage_end"][:-1])
    assert "shape" in P.mismatches(shorter, w)[0]
    t = P.want_of("text_coverage_sam")
    got = {"bedgraph": t["bedgraph"].copy()}
    got["bedgraph"][len(got["bedgraph"]) // 2] ^= 0x20
    assert len(P.mismatches(got, t)) == 1
    c = P.want_of("count_scan_%d" % (P.L.SCAN_BLOCK + 1))
    sse = [k for k in c if k.endswith("_sse3")]
    assert sse and all(c[k].dtype == np.float64 for k in sse)
    nan = {"x_sse3": np.array([0.5, np.nan, 1.0])}
    assert P.mismatches({"x_sse3": nan["x_sse3"].copy()}, nan) == [] and len(P.mismatches({"x_sse3": np.array([0.5, 0.0, 1.0])}, nan)) == 1          # NaN equals NaN only
    got = dict(c)
    got[sse[0]] = c[sse[0]].copy()
    k = int(np.flatnonzero(np.isfinite(got[sse[0]]))[0])
    got[sse[0]][k] = np.nextafter(got[sse[0]][k], 2.0)              # one unit in the last place
    assert [b.split(":")[0] for b in P.mismatches(got, c)] == [sse[0]]
    d = P.want_of("decode_shuffled_all_switches")
    assert d["a_name_key"].dtype == np.uint64 and int(d["a_name_key"][0]) > 2 ** 63          # (beyond int64: compared as it is)
    got = dict(d, a_name_key=d["a_name_key"] ^ np.uint64(1))
    assert [b.split(":")[0] for b in P.mismatches(got, d)] == ["a_name_key"]
    # one base code of a packed genome, one counter of the motif tally, one row of a BED (its strand byte, then its score)
    g = P.want_of("genome_pack_windows")
    got = dict(g, window4096_bases=g["window4096_bases"].copy())
    k = int(np.flatnonzero(got["window4096_bases"] == 1)[1000])
    got["window4096_bases"][k] = 2          # an A read as a C
    bad = P.mismatches(got, g)
    assert len(bad) == 1 and bad[0].startswith("window4096_bases: 1 of %d entries differ, the first at %d: 2 where 1 was expected" % (g["window4096_bases"].size, k))
    m = P.want_of("motif_one_set")
    for key in ("random_tally", "random_tally_again", "planted_strand_tally"):
        got = dict(m)
        got[key] = m[key].copy()
        got[key][7 if key.endswith("tally_again") else 1] *= 2          # (what a tally buffer that is not cleared gives)
        assert [b.split(":")[0] for b in P.mismatches(got, m)] == [key]
    e = P.want_of("end_to_end_junctions_from_motif")
    for column, other in ((3, 63), (4, 0)):
        got = {"bed_rows": e["bed_rows"].copy()}
        row = int(np.flatnonzero(e["bed_rows"][:, 3] == 43)[0])
        got["bed_rows"][row, column] = other
        assert len(P.mismatches(got, e)) == 1
    assert "shape" in P.mismatches({"bed_rows": e["bed_rows"][1:]}, e)[0]


def test_results_come_back_from_the_drivers_file_as_they_went_in(tmp_path):
    for name in ("one_set_every_consumer", "count_scan_%d" % (P.L.SCAN_BLOCK + 1), "decode_shuffled_all_switches", "end_to_end_process_kat2"):
        want = P.want_of(name)
        raw = {k: (v.astype(np.int32) if v.dtype == np.int64 and v.size and abs(v).max() < 2 ** 31 else v) for k, v in want.items()}
        path = str(tmp_path / (name + ".npz"))
        np.savez(path, **raw)
        assert P.mismatches(P.load(path), want) == []


@pytest.mark.parametrize("kept", ["flag", "cigar", "xs", "name_key"])
def test_a_closed_file_lives_as_long_as_any_of_its_views(kept, tmp_path):
    """What the decode case of the list found: its driver closes the file and writes the arrays afterwards, and the name keys -- the
    one array it does not convert on the way -- came back as freed host memory, because the native object was closed when the POS
    view went, whichever views were still alive.  Host decode, no GPU: the object stays parked until the last view is gone."""
    import gc
    from spliser_amd import native
    inp = P.case("decode_sorted_in_three_shares").build(str(tmp_path / "d"))
    bam = native.BamFile(inp["sorted_path"], threads=1, aux_strand=True, mate_keys=True)
    rs = bam.reads("b")
    view, want = getattr(rs, kept), np.array(getattr(rs, kept))
    assert view.size > 1000 and view.base is not None
    before = set(native._BamHandle._parked)
    bam.close()
    parked = set(native._BamHandle._parked) - before
    assert len(parked) == 1
    del rs, bam
    gc.collect()
    assert parked <= set(native._BamHandle._parked)          # POS is gone, the file is not
    assert np.array_equal(view, want)
    del view
    gc.collect()
    assert not parked & set(native._BamHandle._parked)       # the last view is gone: closed
