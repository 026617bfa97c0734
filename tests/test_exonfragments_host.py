"""``exoncounts --countReadPairs`` on the host: the fragment rule (``spl_exon_fragment_rule_host``, the kernel's own header compiled
for the host) against the yardstick of ``exonfragcases.py`` on generated paired content whose coverage is asserted, on the hand
cases and against the gene-level fragment rule; the ascent of one read's bins that the kernel's merge rests on; the rule's header in
a stand-alone program under AddressSanitizer and UBSan (tests/hostsim/exonfragment_rule_asan.cpp); the command line.  No GPU."""
import os
import subprocess
import types

import numpy as np
import pytest

import exoncases as X
import exonfragcases as F
import genecases as G
import matecases as M
from spliser_amd import cli, exoncounts as xc, genecounts as gc, native, samio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTE = {"+": 43, "-": 45, ".": 46}
N_GENES, LENGTH = 9, 6000


def _arrays(features):
    return (np.array([f[0] for f in features], np.int64), np.array([f[1] for f in features], np.int64), np.array([BYTE[f[2]] for f in features], np.uint8),
            np.array([f[3] for f in features], np.int64))


def _labels(features, length, stranded):
    return {w: X.labels_of_features(features, length, w) for w in "+-"} if stranded else X.labels_of_features(features, length)


def _maps(features, stranded):
    a, b, (gene, start, end) = xc.exon_maps(*_arrays(features), stranded=bool(stranded))
    return a, b, list(zip(start.tolist(), end.tolist(), gene.tolist()))


def _hook(rs, mate, bins, a, b, stranded, shift=0, cap=1 << 16):
    arrays = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)
    return native.exon_fragment_rule_host(arrays, np.asarray(mate, np.uint32), np.array([t[2] for t in bins], np.uint32), a, b, stranded, shift, cap)


def _split(verdict, n_hits, flat):
    """The hook's three arrays -> [(verdict, [bins])] per read."""
    out, at = [], 0
    for v, n in zip(verdict.tolist(), n_hits.tolist()):
        out.append((v, flat[at:at + n].tolist()))
        at += n
    assert at == flat.shape[0]
    return out


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


@pytest.fixture(scope="module")
def content():
    """A generated paired set of every kind -- ``matecases``' coverage asserted --, random features, and the yardstick's mate table
    and fragment results (unstranded, fr, rf) in bin numbers, computed once."""
    rng = np.random.default_rng(20261021)
    # random features of every kind on the lower half, and above them three genes of seven exons each with 30 bases between two:
    # mates a few hundred bases apart share a bin, fall into different bins of one gene, or into two genes
    features = G.random_features(rng, 2200, N_GENES, 16)
    features += [(2400 + 770 * g + 110 * j, 2480 + 770 * g + 110 * j, "+-."[g], g) for g in range(3) for j in range(7)]
    records, names, kinds = M.paired_records(rng, 1500, LENGTH - 1200)
    rs = samio.ReadSet.from_records(records)
    keys = np.array([M.name_key(n) for n in names], np.uint64)
    M.assert_covers(kinds, rs.flag, rs.pos, np.diff(rs.cig_off.astype(np.int64)), keys)
    mate, counts = M.mate_table_of(rs, keys)
    out = dict(rs=rs, keys=keys, mate=mate, counts=counts, features=features)
    for stranded in (0, 1, 2):
        labels = _labels(features, LENGTH, stranded)
        a, b, bins = _maps(features, stranded)
        assert bins == X.bins_of([labels["+"], labels["-"]] if stranded else [labels])
        number_of = {key: k for k, key in enumerate(bins)}
        out[stranded] = dict(labels=labels, a=a, b=b, bins=bins, results=F.numbered(F.fragment_results(rs, keys, labels, stranded, mate=mate), number_of))
    return out


def test_the_content_is_not_trivial(content):
    """Said on the yardstick alone: at least 50 fragments of every kind the rule tells apart."""
    rs, mate = content["rs"], content["mate"]
    pos, flag, off, cig = rs.pos.tolist(), rs.flag.tolist(), rs.cig_off.tolist(), rs.cigar.tolist()
    seen = dict.fromkeys(("share a bin", "disjoint bins of one gene", "two genes", "one mate shared", "one mate nowhere, the other counted", "different maps"), 0)
    for stranded in (0, 1):
        labels = content[stranded]["labels"]
        for i, (verdict, _) in enumerate(F.fragment_results(rs, content["keys"], labels, stranded, mate=mate)):
            m = mate[i]
            if verdict in (F.SILENT, F.NOT_COUNTED) or m == M.NONE:
                continue
            (b1, s1), (b2, s2) = (F.under(flag[k], pos[k], cig[off[k]:off[k + 1]], labels, stranded) for k in (i, m))
            if stranded:
                seen["different maps"] += G.read_strand(flag[i], 1) != G.read_strand(flag[m], 1)
                continue
            seen["share a bin"] += verdict == F.COUNTED and bool(set(b1) & set(b2))
            seen["disjoint bins of one gene"] += verdict == F.COUNTED and bool(b1) and bool(b2) and not set(b1) & set(b2)
            seen["two genes"] += not s1 and not s2 and len(set(b1.values())) == 1 and len(set(b2.values())) == 1 and set(b1.values()) != set(b2.values())
            seen["one mate shared"] += s1 != s2
            seen["one mate nowhere, the other counted"] += verdict == F.COUNTED and (not b1 or not b2)
    assert min(seen.values()) >= 50, seen


@pytest.mark.parametrize("stranded", [0, 1, 2])
def test_the_hook_against_the_yardstick(built, content, stranded):
    rs, mate, c = content["rs"], content["mate"], content[stranded]
    verdict, n_hits, flat = _hook(rs, mate, c["bins"], c["a"], c["b"], stranded)
    want = c["results"]
    assert _split(verdict, n_hits, flat) == want
    n_pairs = content["counts"]["paired"] // 2
    # -4 only for a read whose mate has a lower index, and for every such eligible read
    silent = [i for i, (v, _) in enumerate(want) if v == F.SILENT]
    assert len(silent) == n_pairs and all(mate[i] != M.NONE and mate[i] < i for i in silent)
    sums = F.counts_of(want, None, len(c["bins"]))
    assert sum(sums[len(c["bins"]):]) == rs.n - n_pairs and min(sums[len(c["bins"]):]) > 0
    if stranded:
        assert want != content[0]["results"]
    # every hit, also beyond cap; the list as far as cap reaches
    for cap in (0, 1, 7):
        v2, n2, f2 = _hook(rs, mate, c["bins"], c["a"], c["b"], stranded, cap=cap)
        assert v2.tolist() == verdict.tolist() and n2.tolist() == n_hits.tolist() and f2.tolist() == flat[:cap].tolist()
    # moved into a shard: the maps moved by as much
    shift = 700000
    moved = _hook(rs, mate, c["bins"], (c["a"][0] + shift, c["a"][1]), None if c["b"] is None else (c["b"][0] + shift, c["b"][1]), stranded, shift)
    assert _split(*moved) == want


@pytest.mark.parametrize("stranded", [0, 1, 2])
def test_the_verdict_is_the_gene_level_fragment_rules(built, content, stranded):
    rs, mate, c = content["rs"], content["mate"], content[stranded]
    arrays = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar)
    ga, gb = gc.gene_maps(*_arrays(content["features"]), stranded=bool(stranded))
    genes = native.gene_fragment_rule_host(arrays, np.array(mate, np.uint32), N_GENES, ga, gb, stranded).tolist()
    verdict, n_hits, flat = _hook(rs, mate, c["bins"], c["a"], c["b"], stranded)
    at = 0
    for v, n, g in zip(verdict.tolist(), n_hits.tolist(), genes):
        assert v == (F.COUNTED if g >= 0 else g)
        if v == F.COUNTED:
            assert {c["bins"][k][2] for k in flat[at:at + n].tolist()} == {g}
        at += n


def test_fragments_differ_from_reads_where_they_should(built, content):
    """Per read the same set adds two to a bin both mates overlap."""
    c, rs = content[0], content["rs"]
    number_of = {key: k for k, key in enumerate(c["bins"])}
    per_read = X.counts_of(X.reads_of(rs, c["labels"]), number_of, len(c["bins"]))
    per_fragment = F.counts_of(c["results"], None, len(c["bins"]))
    n = len(c["bins"])
    assert sum(per_read[n:]) - sum(per_fragment[n:]) == content["counts"]["paired"] // 2
    assert all(f <= r for f, r in zip(per_fragment[:n], per_read[:n])) and sum(per_fragment[:n]) < sum(per_read[:n])


@pytest.mark.parametrize("stranded", [0, 1])
def test_one_reads_bins_ascend_on_both_maps(built, content, stranded):
    """What the merge rests on: bins are numbered over both maps, so a map's bins ascend along it, and so do one read's."""
    rng = np.random.default_rng(5)
    for seed in range(4):
        features = G.random_features(rng, LENGTH - 1200, 6, 30) if seed else content["features"]
        a, b, bins = _maps(features, stranded)
        bin_gene = np.array([t[2] for t in bins], np.uint32)
        for start, code in ([a, b] if stranded else [a]):
            own = code[(code != 0) & (code != G.MANY)].astype(np.int64)
            assert (np.diff(own) > 0).all()
        none = (np.zeros(0, np.int32), np.zeros(0, np.uint32))
        for flag, pos, cigar in G.random_records(rng, 150, LENGTH - 1200) + [(0, 1, "%dM" % (LENGTH - 1300))]:
            for maps in ((a, b), (b, a)) if stranded else ((a, none),):          # the read's own map, and the other one
                got = native.exon_count_rule_host(flag, pos, G.ops(cigar), bin_gene, maps[0], maps[1], stranded, cap=4096)[1]
                assert all(x < y for x, y in zip(got, got[1:]))


@pytest.mark.parametrize("stranded", [0, 1])
@pytest.mark.parametrize("spread", [0, 70, 300])
def test_the_hand_cases(built, spread, stranded):
    labels = _labels(F.HAND_FEATURES, F.HAND_LENGTH, stranded)
    a, b, bins = _maps(F.HAND_FEATURES, stranded)
    number_of = {key: k for k, key in enumerate(bins)}
    names = sorted(F.HAND_CASES)
    for group in [names] + [[n] for n in names]:          # all together, and each alone
        records, keys, where = F.hand_set(group, spread)
        rs = samio.ReadSet.from_records(records)
        mate = M.mate_table_of(rs, keys)[0]
        assert all(mate[w] == w + spread + 1 for w in where)
        want = [F.HAND_CASES[n][2 + stranded] for n in group]
        results = F.fragment_results(rs, keys, labels, stranded, mate=mate)
        assert [results[w] for w in where] == [(v, sorted(k)) for v, k in want]          # the yardstick says what was read off by hand
        got = _split(*_hook(rs, mate, bins, a, b, stranded))
        assert got == F.numbered(results, number_of)
        assert [got[w][0] for w in where] == [v for v, _ in want] and all(got[w + spread + 1] == (F.SILENT, []) for w in where)
    assert len(F.HAND_CASES["a mate over 70 bins, a one-bin leader"][2][1]) > 70


def test_mate_indexes_the_rule_does_not_believe(built):
    """At or beyond n, or the read itself: no mate."""
    a, b, bins = _maps(F.HAND_FEATURES, 0)
    rs = samio.ReadSet.from_records([(99, 121, "30M"), (147, 141, "30M")])
    for mate in ([2, 0], [0, 0], [0xFFFFFFF0, 0xFFFFFFFF], [7, 1]):
        verdict, n_hits, flat = _hook(rs, mate, bins, a, b, 0)
        if mate[1] == 0:
            assert verdict.tolist() == [0, F.SILENT] and flat.tolist() == [0]
        else:
            assert verdict.tolist() == [0, 0] and flat.tolist() == [0, 0]


def test_hook_refusals(built):
    rs = samio.ReadSet.from_records([(99, 121, "30M"), (147, 141, "30M")])
    genes = [(0, 0, 0), (0, 0, 1)]
    for bad, match in (((np.array([30, 20], np.int32), np.array([1, 2], np.uint32)), "ascending"), ((np.array([20, 30], np.int32), np.array([1, 3], np.uint32)), "code")):
        with pytest.raises(native.SpliserNativeError, match=match) as err:
            _hook(rs, [1, 0], genes, bad, None, 0)
        assert err.value.code == -1
    with pytest.raises(native.SpliserNativeError, match="stranded"):
        _hook(rs, [1, 0], genes, None, None, 3)
    with pytest.raises(ValueError):
        _hook(rs, [1], genes, None, None, 0)


def test_header_under_the_sanitizers(tmp_path, content):
    """The rule's header alone in a program of its own: every array in a heap block of exactly its size, mate tables that point
    beyond the segment and at the read itself, and CIGAR offsets that go down."""
    exe = str(tmp_path / "exonfragment_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostsim", "exonfragment_rule_asan.cpp"), "-o", exe])
    text_of = lambda v: " ".join(str(int(x)) for x in v)
    none = (np.zeros(0, np.int32), np.zeros(0, np.uint32))
    rs = content["rs"]
    lines, want = [], []

    def case(rs, mate, stranded, shift, cap, a, b, bins):
        b = b or none
        lines.append("|".join(["%d %d %d" % (shift, stranded, cap), text_of(rs.pos), text_of(rs.flag), text_of(rs.cig_off), text_of(rs.cigar), text_of(mate), text_of(a[0]), text_of(a[1]),
                               text_of(b[0]), text_of(b[1]), text_of([t[2] for t in bins])]))

    for stranded in (0, 1, 2):
        c = content[stranded]
        for cap in (0, 5, 1 << 16):
            case(rs, content["mate"], stranded, 0, cap, c["a"], c["b"], c["bins"])
            flat = [k for _, keys in c["results"] for k in keys]
            want.append(([v for v, _ in c["results"]], [len(k) for _, k in c["results"]], flat[:cap]))
    # the hand cases: over 70 bins on either mate
    a, b, bins = _maps(F.HAND_FEATURES, 1)
    records, keys, where = F.hand_set(sorted(F.HAND_CASES), 3)
    hand = samio.ReadSet.from_records(records)
    mate = M.mate_table_of(hand, keys)[0]
    number_of = {key: k for k, key in enumerate(bins)}
    results = F.numbered(F.fragment_results(hand, keys, _labels(F.HAND_FEATURES, F.HAND_LENGTH, 1), 1, mate=mate), number_of)
    case(hand, mate, 1, 0, 1 << 16, a, b, bins)
    want.append(([v for v, _ in results], [len(k) for _, k in results], [k for _, keys in results for k in keys]))
    # mate tables the rule does not believe: beyond the segment, the read itself (the program's answer is held against the library's)
    two = samio.ReadSet.from_records([(99, 121, "30M"), (147, 141, "30M"), (99, 2001, F.LONG)])
    for bad in ([3, 0, 2], [0xFFFFFFF0, 1, 0xFFFFFFFE], [2, 1, 0], [1, 2, 0]):
        case(two, bad, 1, 0, 100, a, b, bins)
        v, n, f = _hook(two, bad, bins, a, b, 1, cap=100)
        want.append((v.tolist(), n.tolist(), f.tolist()))
    # CIGAR offsets that go down, and one beyond the ops: such a read has no op and is not counted
    down = types.SimpleNamespace(pos=[121, 141, 161], flag=[99, 147, 0], cig_off=[2, 1, 9, 3], cigar=[30 << 4] * 3)
    case(down, [1, 0, M.NONE], 0, 0, 10, a, None, bins)
    want.append(([F.NOT_COUNTED] * 3, [0, 0, 0], []))
    # a read at the top of the coordinate space with a shift on top, a map of one entry, and no read at all
    top = samio.ReadSet.from_records([(99, 2147483000, "1000M"), (147, 2147483000, "1000M")])
    case(top, [1, 0], 0, 500000, 4, (np.array([2147483500], np.int32), np.array([1], np.uint32)), None, [(0, 0, 0)])
    want.append(([0, F.SILENT], [1, 0], [0]))
    lines.append("|".join(["0 0 0", "", "", "0", "", "", "", "", "", "", ""]))
    want.append(([], [], []))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stderr
    got = out.stdout.split("\n")
    assert len(got) >= 3 * len(want)
    for k, (verdict, n_hits, flat) in enumerate(want):
        assert [int(v) for v in got[3 * k].split()] == verdict, k
        assert [int(v) for v in got[3 * k + 1].split()] == n_hits, k
        assert [int(v) for v in got[3 * k + 2].split()] == flat, k
    assert max(max(w[1]) for w in want if w[1]) > 70


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_the_switch_is_exoncounts_alone(capsys):
    p = cli.build_parser()
    assert "countReadPairs" not in vars(p.parse_args(["exoncounts", "-B", "x", "-A", "g", "-o", "o"]))          # without it, the arguments are what they were
    assert vars(p.parse_args(["exoncounts", "-B", "x", "-A", "g", "-o", "o", "--countReadPairs"]))["countReadPairs"] is True
    for command in ("process", "junctions", "coverage", "strandedness", "flagstat", "intronretention", "genecounts"):
        with pytest.raises(SystemExit):
            p.parse_args([command, "-B", "x", "-A", "g", "-o", "o", "--countReadPairs"])
    capsys.readouterr()
    with pytest.raises(SystemExit) as err:
        cli.main(["exoncounts", "-B", "x.bam", "-A", "g.gtf", "-o", "o", "--fragments"])
    text = capsys.readouterr().err
    assert err.value.code == 2 and "genecounts --fragments" in text and "--countReadPairs" in text
    with pytest.raises(SystemExit):          # ... also beside the right switch
        cli.main(["exoncounts", "-B", "x.bam", "-A", "g.gtf", "-o", "o", "--fragments", "--countReadPairs"])
    assert "--countReadPairs" in capsys.readouterr().err


def test_the_function_takes_the_switch_and_refuses_a_source_without_keys():
    import inspect
    assert inspect.signature(xc.exoncounts).parameters["countReadPairs"].default is False
    assert inspect.signature(xc.counts_of_source).parameters["fragments"].default is False

    class NoKeys(object):
        mate_keys = False
        ref_names = []
    with pytest.raises(native.SpliserNativeError, match="name keys"):
        xc.counts_of_source(NoKeys(), (0,), [], None, fragments=True)

    class Shares(object):
        mate_keys = True
        shares = [(0, ["c1"]), (1, ["c1"])]
    with pytest.raises(native.SpliserNativeError, match="one device"):
        xc.counts_of_source(Shares(), (0,), [], None, fragments=True)
