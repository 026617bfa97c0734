"""``saturation`` and ``junctions --subsample`` against the unchanged commands on pre-subsampled files: a paired, named file of a few
thousand reads; for K = 4 and one seed the four files that hold exactly the reads the restatement (``subsamplecases.py``) keeps at
T_k are written with ``samio.write_bam``, ``junctions`` and ``process`` (without ``-b``, without ``-A``) run on each, and every row of
``saturation.tsv`` is the six numbers derived from their files.  The input as BAM on the device, BAM on the host threads, SAM text,
BGZF SAM text and the BAM shuffled gives one byte-identical table."""
import numpy as np
import pytest

import matecases as M
import samzcases as Z
import subsamplecases as S
from spliser_amd import cli, samio

pytestmark = pytest.mark.gpu

NAMES, LENGTHS, SPAN = ["c1", "c2", "c3"], [10 ** 6] * 3, 3000
K, SEED, MIN_READS = 4, 11, 10


def _masked(rs, names, mask):
    n_ops = np.diff(rs.cig_off.astype(np.int64))
    out = samio.ReadSet(rs.pos[mask], rs.flag[mask], np.concatenate(([0], np.cumsum(n_ops[mask]))), rs.cigar[np.repeat(mask, n_ops)])
    return out, [nm for nm, m in zip(names, mask) if m]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Three chromosomes (the third without a read) of generated paired reads with names, of every kind ``matecases`` knows; the one
    content in five forms, and per step the file of the reads the restatement keeps."""
    d = tmp_path_factory.mktemp("saturation")
    rng = np.random.default_rng(43)
    sets, names, kinds = [], [], set()
    for chrom in NAMES[:2]:
        records, nm, kd = M.paired_records(rng, 1500, SPAN)
        kinds |= kd
        keep = [j for j, r in enumerate(records) if r[1] >= 1]          # (a file has no POS 0 on a reference)
        sets.append((chrom, samio.ReadSet.from_records([records[j] for j in keep])))
        names.append([nm[j] for j in keep])
    assert M.KINDS - {"POS 0"} <= kinds
    bam, shuffled, sam, samz = str(d / "p.bam"), str(d / "s.bam"), str(d / "p.sam"), str(d / "p.sam.gz")
    samio.write_bam(bam, NAMES, LENGTHS, sets, with_seq=True, unplaced=3, names=names)
    singles = [(chrom, rs.take(j, j + 1), [nm[j]]) for (chrom, rs), nm in zip(sets, names) for j in range(rs.n)]
    order = rng.permutation(len(singles))
    samio.write_bam(shuffled, NAMES, LENGTHS, [singles[j][:2] for j in order], with_seq=True, names=[singles[j][2] for j in order])
    samio.write_sam(sam, NAMES, LENGTHS, sets, names=names)
    with open(sam, "rb") as fh, open(samz, "wb") as out:
        out.write(Z.bgzf(fh.read(), block=0xff00))
    keys = [np.array([M.name_key(n) for n in nm], np.uint64) for nm in names]

    def kept_file(path, seed, threshold):
        kept, kept_names, n = [], [], 0
        for (chrom, rs), nm, ky in zip(sets, names, keys):
            mask = S.keep_mask(ky, rs.pos, rs.flag, np.diff(rs.cig_off.astype(np.int64)), seed, threshold)
            sub, sub_names = _masked(rs, nm, mask)
            kept.append((chrom, sub))
            kept_names.append(sub_names)
            n += sub.n
        samio.write_bam(path, NAMES, LENGTHS, kept, with_seq=True, names=kept_names)
        return n

    steps = []
    for k, threshold in enumerate(S.thresholds(K), 1):
        path = str(d / ("step%d.bam" % k))
        steps.append((path, kept_file(path, SEED, threshold)))
    half = str(d / "half.bam")
    n_half = kept_file(half, 3, int(0.5 * 4294967296.0))
    return dict(dir=str(d), bam=bam, shuffled=shuffled, sam=sam, samz=samz, steps=steps, half=half, n_half=n_half, n=sum(rs.n for _, rs in sets))


def _six_numbers(bam, n_reads, prefix, extra=()):
    """The unchanged ``junctions`` and ``process`` on ``bam`` -> the row's six numbers, from their files."""
    assert cli.main(["junctions", "-B", bam, "-o", prefix + ".bed"] + list(extra)) == 0
    assert cli.main(["process", "-B", bam, "-o", prefix] + list(extra)) == 0
    scores = [int(line.split("\t")[4]) for line in open(prefix + ".bed") if not line.startswith("track")]
    lines = open(prefix + ".SpliSER.tsv").read().splitlines()
    head = lines[0].split("\t")
    cols = [head.index(c) for c in ("alpha_count", "beta1_count", "beta2Simple_count")]
    totals = [sum(int(line.split("\t")[c]) for c in cols) for line in lines[1:]]
    return (n_reads, len(scores), sum(1 for s in scores if s >= MIN_READS), sum(scores), len(totals), sum(1 for t in totals if t >= MIN_READS))


def _table(path):
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == ["step", "fraction", "reads", "junctions", "junctions_minReads", "junction_reads", "sites", "sites_minReads"]
    return [tuple(line.split("\t")) for line in lines[1:]]


@pytest.fixture(scope="module")
def wanted(files):
    return [_six_numbers(path, n, "%s/want%d" % (files["dir"], k)) for k, (path, n) in enumerate(files["steps"], 1)]


def test_every_row_is_the_three_commands_on_the_pre_subsampled_file(files, wanted, capsys):
    d = files["dir"]
    assert cli.main(["saturation", "-B", files["bam"], "-o", d + "/bam", "--steps", str(K), "--seed", str(SEED)]) == 0
    log = capsys.readouterr().out
    rows = _table(d + "/bam.saturation.tsv")
    assert len(rows) == K
    for k, (row, want) in enumerate(zip(rows, wanted), 1):
        assert row[0] == str(k) and row[1] == repr(k / K)
        assert tuple(int(v) for v in row[2:]) == want, k
    # row K is the plain, full-depth process and junctions on the file itself
    assert tuple(int(v) for v in rows[-1][2:]) == _six_numbers(files["bam"], files["n"], d + "/whole")
    # nothing falls from one row to the next, and the rows differ
    for a, b in zip(wanted, wanted[1:]):
        assert a[0] <= b[0] and a[1] <= b[1] and a[4] <= b[4]
    assert 0 < wanted[0][0] < wanted[1][0] < wanted[2][0] < wanted[3][0] == files["n"] and 0 < wanted[0][1] < wanted[3][1]
    assert 0 < wanted[3][5] < wanted[3][4] and wanted[0][5] < wanted[3][5]
    assert "step 1 of 4" in log and "step 4 of 4" in log
    assert ("sites with at least %d reads: %d at full depth, %d (" % (MIN_READS, wanted[3][5], wanted[1][5])) in log and "at half the depth" in log


def test_five_forms_of_the_input_give_one_table(files, capsys):
    d = files["dir"]
    runs = [("dev", ["-B", files["bam"]]), ("host", ["-B", files["bam"], "--hostDecode"]), ("sam", ["-B", files["sam"]]), ("samz", ["-B", files["samz"]]),
            ("shuffled", ["-B", files["shuffled"], "--anyOrder"])]
    texts = {}
    for tag, args in runs:
        assert cli.main(["saturation", "-o", d + "/" + tag, "--steps", str(K), "--seed", str(SEED)] + args) == 0
        texts[tag] = open("%s/%s.saturation.tsv" % (d, tag), "rb").read()
    capsys.readouterr()
    assert len(set(texts.values())) == 1 and texts["dev"].count(b"\n") == K + 1
    # another seed keeps other reads; one chromosome is its rows alone; stranded rows differ from unstranded ones
    assert cli.main(["saturation", "-B", files["bam"], "-o", d + "/seed", "--steps", str(K), "--seed", "12"]) == 0
    other = _table(d + "/seed.saturation.tsv")
    assert other[-1] == _table(d + "/dev.saturation.tsv")[-1] and other[0] != _table(d + "/dev.saturation.tsv")[0]


def test_one_chromosome_stranded_and_filtered_rows(files, capsys):
    d = files["dir"]
    extra = ["-c", "c2", "--isStranded", "-s", "fr", "--excludeFlags", "0x900", "--minAnchor", "10", "--minIntron", "75", "--maxIntron", "150"]
    assert cli.main(["saturation", "-B", files["bam"], "-o", d + "/c2", "--steps", "2", "--seed", str(SEED), "-r", "3"] + extra) == 0
    capsys.readouterr()
    rows = _table(d + "/c2.saturation.tsv")
    assert cli.main(["junctions", "-B", files["bam"], "-o", d + "/c2.bed"] + extra) == 0
    assert cli.main(["process", "-B", files["bam"], "-o", d + "/c2"] + extra) == 0
    scores = [int(line.split("\t")[4]) for line in open(d + "/c2.bed") if not line.startswith("track")]
    sites = open(d + "/c2.SpliSER.tsv").read().splitlines()[1:]
    totals = [sum(int(line.split("\t")[c]) for c in (5, 6, 7)) for line in sites]
    assert tuple(int(v) for v in rows[-1][3:]) == (len(scores), sum(1 for s in scores if s >= 3), sum(scores), len(sites), sum(1 for t in totals if t >= 3))
    assert 0 < int(rows[0][2]) < int(rows[1][2]) < files["n"] and len(scores) > 0


def test_junctions_subsample_writes_what_junctions_writes_of_the_pre_subsampled_file(files, capsys):
    d = files["dir"]
    assert cli.main(["junctions", "-B", files["half"], "-o", d + "/half.want.bed"]) == 0
    capsys.readouterr()
    want = open(d + "/half.want.bed", "rb").read()
    for tag, args in (("dev", ["-B", files["bam"]]), ("sam", ["-B", files["sam"]]), ("samz", ["-B", files["samz"]]), ("shuffled", ["-B", files["shuffled"], "--anyOrder"])):
        assert cli.main(["junctions", "-o", "%s/half.%s.bed" % (d, tag), "--subsample", "0.5", "--seed", "3"] + args) == 0
        log = capsys.readouterr().out
        assert open("%s/half.%s.bed" % (d, tag), "rb").read() == want, tag
        assert ("(subsample: %d of %d reads kept, fraction 0.5, seed 3)" % (files["n_half"], files["n"])) in log
    assert want.count(b"\n") > 10
    # without the switch the command writes what it wrote and says nothing of a subsample; a fraction of 1 keeps every read
    assert cli.main(["junctions", "-B", files["bam"], "-o", d + "/plain.bed"]) == 0
    assert "subsample" not in capsys.readouterr().out
    assert cli.main(["junctions", "-B", files["bam"], "-o", d + "/one.bed", "--subsample", "1"]) == 0
    assert ("(subsample: %d of %d reads kept, fraction 1.0, seed 0)" % (files["n"], files["n"])) in capsys.readouterr().out
    plain = open(d + "/plain.bed", "rb").read()
    assert plain == open(d + "/one.bed", "rb").read() and plain != want


def test_host_decode_gives_the_device_decodes_table(files, capsys):
    d = files["dir"]
    for tag, args in (("r3dev", []), ("r3host", ["--hostDecode"])):
        assert cli.main(["saturation", "-B", files["bam"], "-o", d + "/" + tag, "--steps", "3", "-r", "2"] + args) == 0
    capsys.readouterr()
    assert open(d + "/r3dev.saturation.tsv", "rb").read() == open(d + "/r3host.saturation.tsv", "rb").read()
