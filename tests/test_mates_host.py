"""Mate pairing and fragment counting without a GPU: the name key of the library, of ``samio`` and of the yardstick
(``matecases.py``) on names of every kind; the keys the host decoders leave beside FLAG -- BAM under a filter, with unplaced records
and sorted from a shuffled file, SAM text plain and compressed -- against the written names; the pair stage's host form and the
fragment rule on the host against the yardstick on generated paired sets, whose coverage is asserted; and the rule's header in a
stand-alone program under AddressSanitizer and UBSan (tests/hostsim/mate_rule_asan.cpp)."""
import gzip
import os
from contextlib import closing
import subprocess

import numpy as np
import pytest

import genecases as G
import matecases as M
from spliser_amd import genecounts as gc, native, process as proc, samio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTE = {"+": 43, "-": 45, ".": 46}
NAMES = list(M.SPECIAL_NAMES) + [b"r0", b"frag:17/x", b"A" * 253, b"\x80", b"\xff" * 7, b"**", b"* ", bytes(range(1, 255))]
N_GENES, LENGTH = 9, 6000


def _arrays(features):
    return (np.array([f[0] for f in features], np.int64), np.array([f[1] for f in features], np.int64), np.array([BYTE[f[2]] for f in features], np.uint8),
            np.array([f[3] for f in features], np.int64))


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


@pytest.fixture(scope="module")
def content():
    """A generated paired set of every kind on 6000 bases -- its coverage asserted -- random features with their three maps, and the
    yardstick's mate table and fragment results (unstranded, fr, rf), computed once."""
    rng = np.random.default_rng(20261020)
    features = G.random_features(rng, LENGTH - 1200, N_GENES, 30)
    records, names, kinds = M.paired_records(rng, 400, LENGTH - 1200)
    rs = samio.ReadSet.from_records(records)
    keys = np.array([M.name_key(n) for n in names], np.uint64)
    M.assert_covers(kinds, rs.flag, rs.pos, np.diff(rs.cig_off.astype(np.int64)), keys)
    a, _ = gc.gene_maps(*_arrays(features))
    plus, minus = gc.gene_maps(*_arrays(features), stranded=True)
    bases = G.bases_of_features(features, LENGTH)
    both = {w: G.bases_of_features(features, LENGTH, w) for w in "+-"}
    mate, counts = M.mate_table_of(rs, keys)
    results = {0: M.fragment_results(rs, keys, bases, mate=mate), 1: M.fragment_results(rs, keys, both, 1, mate=mate), 2: M.fragment_results(rs, keys, both, 2, mate=mate)}
    return dict(rs=rs, names=names, keys=keys, a=a, plus=plus, minus=minus, bases=bases, both=both, mate=mate, counts=counts, results=results)


# ---- the key ------------------------------------------------------------------------------------------------------------------
def test_the_three_keys_agree_on_names_of_every_kind(built):
    assert {len(n) for n in NAMES} >= {0, 1, 254} and any(max(n) >= 0x80 for n in NAMES if n)
    keys = [M.name_key(n) for n in NAMES]
    assert [native.name_key_host(n) for n in NAMES] == keys
    assert [samio.name_key(n) for n in NAMES] == keys
    assert keys[0] == 0 and keys[1] == 0 and all(k != 0 and 0 < k < 2 ** 64 for k in keys[2:])
    assert len(set(keys[2:])) == len(keys) - 2


def test_the_key_is_fnv1a_and_the_finisher_by_the_issues_numbers():
    """The recipe once more, step by step on one name, against the yardstick."""
    h = 0xcbf29ce484222325
    for b in b"read/1":
        h = ((h ^ b) * 0x100000001b3) % 2 ** 64
    for mult in (0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53):
        h ^= h >> 33
        h = h * mult % 2 ** 64
    h ^= h >> 33
    assert M.name_key(b"read/1") == h


# ---- the rule on the host -----------------------------------------------------------------------------------------------------
def test_the_pair_stage_on_the_host_against_the_yardstick(built, content):
    rs, keys = content["rs"], content["keys"]
    arrays = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)
    mate, counts = native.mate_table_host(arrays, keys)
    assert mate.tolist() == content["mate"] and counts == content["counts"]
    assert counts["paired"] % 2 == 0 and 0 < counts["unpaired_mate_mapped"] < counts["pairable"] - counts["paired"]
    m = mate.astype(np.int64)
    has = m != M.NONE
    assert (m[m[has]] == np.nonzero(has)[0]).all()          # symmetric


def test_the_pair_stage_on_groups_of_every_shape(built):
    """Keys given directly: one group of many unequal halves, keys that differ in bit 0 only, the greatest and the least key."""
    rng = np.random.default_rng(3)
    n = 3000
    flag = np.where(rng.random(n) < 0.4, 99, 147).astype(np.uint16)
    rs = samio.ReadSet(np.arange(1, n + 1), flag, np.arange(n + 1), np.full(n, (10 << 4), np.uint32))
    for keys in (np.full(n, 0x123456789abcdef0, np.uint64), rng.integers(2, 4, n).astype(np.uint64), np.where(rng.random(n) < 0.5, 1, 2 ** 64 - 1).astype(np.uint64),
                 rng.integers(1, 40, n).astype(np.uint64) << np.uint64(56)):
        want, want_counts = M.mate_table_of(rs, keys)
        mate, counts = native.mate_table_host(native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar), keys)
        assert mate.tolist() == want and counts == want_counts and counts["paired"] > 0


@pytest.mark.parametrize("stranded", [0, 1, 2])
def test_the_fragment_rule_on_the_host_against_the_yardstick(built, content, stranded):
    rs = content["rs"]
    arrays = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)
    maps = (content["plus"], content["minus"]) if stranded else (content["a"], None)
    got = native.gene_fragment_rule_host(arrays, np.array(content["mate"], np.uint32), N_GENES, maps[0], maps[1], stranded)
    want = content["results"][stranded]
    assert got.tolist() == want
    n_pairs = content["counts"]["paired"] // 2
    assert want.count(M.SILENT) == n_pairs and sum(M.counts_of(want, N_GENES)) == rs.n - n_pairs
    assert min(M.counts_of(want, N_GENES)[N_GENES:]) > 0
    if stranded:
        assert want != content["results"][0]
    # moved into a shard: the map moved by as much
    shift = 700000
    moved = native.gene_fragment_rule_host(arrays, np.array(content["mate"], np.uint32), N_GENES, (maps[0][0] + shift, maps[0][1]),
                                           None if maps[1] is None else (maps[1][0] + shift, maps[1][1]), stranded, shift)
    assert moved.tolist() == want


def test_fragments_differ_from_reads_where_they_should(built, content):
    """Per read the same set comes to other numbers: a pair is two there."""
    rs = content["rs"]
    per_read = G.counts_of(G.results_of(rs, content["bases"]), N_GENES)
    per_fragment = M.counts_of(content["results"][0], N_GENES)
    assert sum(per_read) - sum(per_fragment) == content["counts"]["paired"] // 2 and per_read[N_GENES + 2] == per_fragment[N_GENES + 2]


def test_header_under_the_sanitizers(tmp_path, content):
    """The rule's header alone in a program of its own: every array in a heap block of exactly its size."""
    exe = str(tmp_path / "mate_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostsim", "mate_rule_asan.cpp"), "-o", exe])
    text_of = lambda v: " ".join(str(int(x)) for x in v)
    names_hex = " ".join(n.hex() if n else "-" for n in NAMES)
    lines, want = [], []
    none = (np.zeros(0, np.int32), np.zeros(0, np.uint32))
    for stranded, shift in ((0, 0), (1, 0), (2, 0)):
        rs = content["rs"]
        ma, mb = (content["plus"], content["minus"]) if stranded else (content["a"], none)
        lines.append("|".join(["%d %d" % (shift, stranded), text_of(rs.pos), text_of(rs.flag), text_of(rs.cig_off), text_of(rs.cigar), text_of(content["keys"]), text_of(ma[0]),
                               text_of(ma[1]), text_of(mb[0]), text_of(mb[1]), names_hex]))
        want.append((content["mate"], content["results"][stranded]))
    # one read, and none
    one = samio.ReadSet.from_records([(99, 5, "10M")])
    lines.append("|".join(["0 0", "5", "99", "0 1", text_of(one.cigar), str(2 ** 64 - 1), "", "", "", "", names_hex]))
    want.append(([M.NONE], [G.NO_FEATURE]))
    lines.append("|".join(["0 0", "", "", "0", "", "", "", "", "", "", names_hex]))
    want.append(([], []))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stderr
    got = out.stdout.split("\n")
    assert len(got) >= 3 * len(want)
    for k, (mate, results) in enumerate(want):
        assert [int(v) for v in got[3 * k].split()] == mate
        assert [int(v) for v in got[3 * k + 1].split()] == results
        assert [int(v) for v in got[3 * k + 2].split()] == [M.name_key(n) for n in NAMES]


# ---- the keys the host decoders leave ---------------------------------------------------------------------------------------------
CHROMS, LENGTHS = ["c1", "c2"], [10 ** 6] * 2


@pytest.fixture(scope="module")
def paired_files(tmp_path_factory, built):
    """Two chromosomes of generated paired reads with their names, as BAM (with unplaced records), as the same BAM shuffled record by
    record, as SAM text and as gzip'd SAM text.  (The text forms leave out nothing: an empty QNAME is an empty column 1.)"""
    d = tmp_path_factory.mktemp("mates")
    rng = np.random.default_rng(77)
    sets, names = [], []
    for chrom in CHROMS:
        records, nm, kinds = M.paired_records(rng, 120, 4000)
        keep = [k for k, r in enumerate(records) if r[1] >= 1]          # (a file has no POS 0 on a reference)
        sets.append((chrom, samio.ReadSet.from_records([records[k] for k in keep])))
        names.append([nm[k] for k in keep])
    bam, shuffled, sam, samgz = str(d / "p.bam"), str(d / "s.bam"), str(d / "p.sam"), str(d / "p.sam.gz")
    samio.write_bam(bam, CHROMS, LENGTHS, sets, with_seq=True, unplaced=3, names=names)
    singles = [(chrom, rs.take(k, k + 1), [nm[k]]) for (chrom, rs), nm in zip(sets, names) for k in range(rs.n)]
    order = rng.permutation(len(singles))
    samio.write_bam(shuffled, CHROMS, LENGTHS, [singles[k][:2] for k in order], with_seq=True, names=[singles[k][2] for k in order])
    samio.write_sam(sam, CHROMS, LENGTHS, sets, names=names)
    with open(sam, "rb") as fh, gzip.open(samgz, "wb") as out:
        out.write(fh.read())
    keys = [np.array([M.name_key(n) for n in nm], np.uint64) for nm in names]
    return dict(bam=bam, shuffled=shuffled, sam=sam, samgz=samgz, sets=sets, names=names, keys=keys)


def test_default_names_are_unchanged_and_names_are_written_as_given(tmp_path, paired_files):
    rs = paired_files["sets"][0][1].take(0, 5)
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    samio.write_bam(a, CHROMS, LENGTHS, [("c1", rs)])
    samio.write_bam(b, CHROMS, LENGTHS, [("c1", rs)], names=[[b"r%d" % k for k in range(5)]])
    assert open(a, "rb").read() == open(b, "rb").read()
    samio.write_sam(a, CHROMS, LENGTHS, [("c1", rs)])
    samio.write_sam(b, CHROMS, LENGTHS, [("c1", rs)], names=[[b"r%d" % k for k in range(5)]])
    assert open(a, "rb").read() == open(b, "rb").read()
    with pytest.raises(ValueError):
        samio.write_bam(b, CHROMS, LENGTHS, [("c1", rs)], names=[[b"x"] * 4])
    with pytest.raises(ValueError):
        samio.write_bam(b, CHROMS, LENGTHS, [("c1", rs)], names=[[b"x" * 255] * 5])


@pytest.mark.parametrize("exclude", [0, 0x900])
def test_host_bam_decoder_keys_in_file_order_under_a_filter(paired_files, exclude):
    f = paired_files
    with closing(native.BamFile(f["bam"], threads=2, exclude_flags=exclude, mate_keys=True)) as bam:
        for (chrom, rs), keys in zip(f["sets"], f["keys"]):
            keep = (rs.flag & exclude) == 0
            got = bam.reads(chrom)
            assert got.n == int(keep.sum()) and np.array_equal(got.flag, rs.flag[keep]) and np.array_equal(got.pos, rs.pos[keep])
            assert got.name_key.dtype == np.uint64 and np.array_equal(got.name_key, keys[keep])
            if exclude:
                assert got.n < rs.n
            assert (got.name_key == 0).sum() >= 2          # the nameless ones


def test_host_bam_decoder_sorts_the_keys_with_the_reads(paired_files):
    f = paired_files
    with closing(native.BamFile(f["shuffled"], threads=2, any_order=True, mate_keys=True)) as bam:
        for (chrom, rs), keys in zip(f["sets"], f["keys"]):
            got = bam.reads(chrom)
            # sorted by POS, ties in the shuffled file's order: every (POS, flag, key) as often as written, POS ascending
            assert got.n == rs.n and (np.diff(got.pos.astype(np.int64)) >= 0).all()
            assert sorted(zip(got.pos.tolist(), got.flag.tolist(), got.name_key.tolist())) == sorted(zip(rs.pos.tolist(), rs.flag.tolist(), keys.tolist()))
    # ties in file order: against a stable sort of the shuffled file as it was written
    names_by_chrom = {c: [] for c in CHROMS}
    with closing(native.BamFile(f["shuffled"], threads=1, mate_keys=True)) as plain:          # (no sort: the references' parts in file order)
        for chrom in CHROMS:
            names_by_chrom[chrom] = plain.reads(chrom)
    with closing(native.BamFile(f["shuffled"], threads=2, any_order=True, mate_keys=True)) as bam:
        for chrom in CHROMS:
            raw, got = names_by_chrom[chrom], bam.reads(chrom)
            order = np.argsort(raw.pos, kind="stable")
            assert np.array_equal(got.name_key, raw.name_key[order]) and np.array_equal(got.flag, raw.flag[order])


@pytest.mark.parametrize("which", ["sam", "samgz"])
def test_host_sam_parser_and_the_python_reader_agree(paired_files, which):
    f = paired_files
    _, sets = samio.read_sam(f[which], mate_keys=True)
    with closing(native.SamFile(f[which], threads=2, mate_keys=True)) as sf:
        for (chrom, rs), keys in zip(f["sets"], f["keys"]):
            got = sf.reads(chrom)
            assert sf.decline_reason() in (None, "")
            order = np.argsort(rs.pos, kind="stable")          # (text is always read as in any order; the sets are sorted already)
            assert np.array_equal(order, np.arange(rs.n))
            assert np.array_equal(sets[chrom].name_key, keys) and np.array_equal(got.name_key, keys) and np.array_equal(got.flag, rs.flag)


def test_a_decode_without_the_switch_leaves_no_keys(paired_files, tmp_path):
    f = paired_files
    with closing(native.BamFile(f["bam"], threads=2)) as bam:
        assert bam.reads("c1").name_key is None
        out = native.ctypes.c_void_p(1)
        native._check(native.lib().spl_bam_mate_keys(bam._h, 0, native.ctypes.byref(out)))
        assert not out.value
    with closing(native.SamFile(f["sam"], threads=1)) as sf:
        assert sf.reads("c1").name_key is None
    plain = str(tmp_path / "plain.sam")
    samio.write_sam(plain, CHROMS, LENGTHS, f["sets"])
    assert samio.read_sam(plain)[1]["c1"].name_key is None
    assert samio.read_sam(plain, mate_keys=True)[1]["c1"].name_key[:2].tolist() == [M.name_key(b"r0"), M.name_key(b"r1")]
    src = proc.open_alignments(f["sam"], options=proc.DecodeOptions(mate_keys=True))
    assert np.array_equal(src.reads("c2").name_key, f["keys"][1]) and src.mate_keys


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_the_flag_is_genecounts_alone(capsys):
    from spliser_amd import cli
    p = cli.build_parser()
    assert vars(p.parse_args(["genecounts", "-B", "x", "-A", "g", "-o", "o"]))["fragments"] is False
    assert vars(p.parse_args(["genecounts", "-B", "x", "-A", "g", "-o", "o", "--fragments"]))["fragments"] is True
    for command in ("process", "junctions", "coverage", "strandedness", "flagstat", "intronretention"):
        with pytest.raises(SystemExit):
            p.parse_args([command, "-B", "x", "-o", "o", "--fragments"])
    capsys.readouterr()
    with pytest.raises(SystemExit):          # exon bins are per read: said, not ignored
        cli.main(["exoncounts", "-B", "x.bam", "-A", "g.gtf", "-o", "o", "--fragments"])
    assert "genecounts --fragments" in capsys.readouterr().err
    assert proc.DecodeOptions().mate_keys is False and proc.DecodeOptions(mate_keys=True).mate_keys is True
