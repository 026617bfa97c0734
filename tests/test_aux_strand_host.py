"""The aux walk that gives a spliced read its strand byte (``--strandFromXS``; spl_bam_aux.h), without a GPU: the library's hook
against a walk written here from the SAM specification (``xscases.py_walk``) on hand-built areas; the same header in a stand-alone
program under AddressSanitizer and UBSan over areas cut off at every byte; the host decoder's fifth array against what was
written; SAM text by the same rule."""
import os
import struct
import subprocess

import numpy as np
import pytest

import xscases as X
from spliser_amd import native, samio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLUS, MINUS = ord("+"), ord("-")


@pytest.fixture(scope="module", autouse=True)
def _built():
    native.build()


def _b(sub, values):
    fmt = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[sub]
    return X.field(b"ZB", "B", struct.pack("<%d%s" % (len(values), fmt), *values), sub=sub)


EVERY_TYPE = (X.field(b"aA", "A", b"q") + X.field(b"ac", "c", b"\xff") + X.field(b"aC", "C", b"\x07") + X.field(b"as", "s", b"\x01\x80")
              + X.field(b"aS", "S", b"\xff\xff") + X.field(b"ai", "i", struct.pack("<i", -5)) + X.field(b"aI", "I", struct.pack("<I", 1 << 31))
              + X.field(b"af", "f", struct.pack("<f", 1.5)) + X.field(b"aZ", "Z", b"hello world") + X.field(b"aH", "H", b"1AE301")
              + b"".join(_b(sub, [1, 2, 3]) + _b(sub, []) for sub in "cCsSiIf"))

HAND_BUILT = [
    ("every type, then the tag", EVERY_TYPE + b"XSA-", MINUS),
    ("every type, no tag", EVERY_TYPE, 0),
    ("first", b"XSA+" + EVERY_TYPE, PLUS),
    ("middle", b"NHC\x01" + b"XSA-" + b"ASC\x10", MINUS),
    ("last", X.star_area(b"+"), PLUS),
    ("XS:i before XS:A", b"XSi" + struct.pack("<i", 43) + b"XSA+", PLUS),
    ("XS:i alone", b"XSi" + struct.pack("<i", 43), 0),
    ("XS:Z before XS:A", b"XSZ+\x00" + b"XSA-", MINUS),
    ("XS:A:.", X.star_area(b"."), 0),
    ("XS:A:?", X.star_area(b"?"), 0),
    ("XS:A:. then XS:A:+", b"XSA." + b"XSA+", 0),
    ("two XS:A", b"XSA-" + b"XSA+", MINUS),
    ("bytes in a Z string", b"COZXSA+\x00", 0),
    ("bytes in a Z string, then the tag", b"COZXSA+\x00" + b"XSA-", MINUS),
    ("bytes in a B:C array", b"ZBBC" + struct.pack("<I", 4) + b"XSA+", 0),
    ("bytes in a B:C array, then the tag", b"ZBBC" + struct.pack("<I", 4) + b"XSA+" + b"XSA-", MINUS),
    ("empty", b"", 0),
    ("unknown type", b"abd" + b"\x00" * 8 + b"XSA+", 0),
    ("unknown B subtype", b"ZBBd" + struct.pack("<I", 0) + b"XSA+", 0),
    ("no NUL", b"COZabc", 0),
    ("B count past the end", b"ZBBI" + struct.pack("<I", 0x40000000) + b"XSA+", 0),
    ("B count of all ones", b"ZBBI" + struct.pack("<I", 0xFFFFFFFF) + b"XSA+", 0),
]


@pytest.mark.parametrize("name,aux,want", HAND_BUILT, ids=[h[0] for h in HAND_BUILT])
def test_hook_on_hand_built_areas(name, aux, want):
    assert X.py_walk(aux) == want            # (the yardstick itself says what the issue says)
    assert native.aux_strand_host(aux) == want


def test_hook_on_an_area_cut_off_at_every_byte():
    for xs in (b"+", b"-"):
        full = X.star_area(xs)
        for cut in range(len(full) + 1):
            got = native.aux_strand_host(full[:cut])
            assert got == X.py_walk(full[:cut]) and got == (ord(xs) if cut == len(full) else 0), cut
    for cut in range(len(EVERY_TYPE) + 5):
        area = (EVERY_TYPE + b"XSA-")[:cut]
        assert native.aux_strand_host(area) == X.py_walk(area), cut


def test_hook_on_random_well_formed_areas():
    rng = np.random.default_rng(20261017)
    seen = set()
    for _ in range(4000):
        aux = X.random_area(rng)
        want = X.py_walk(aux)
        seen.add(want)
        assert native.aux_strand_host(aux) == want, aux
    assert seen == {0, PLUS, MINUS}


def test_header_under_the_sanitizers_over_cut_off_areas(tmp_path):
    """The header alone in a program of its own (tests/hostsim/aux_strand_asan.cpp), every cut in a heap block of exactly its size:
    a read at or beyond the end aborts the child."""
    exe = str(tmp_path / "aux_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostsim", "aux_strand_asan.cpp"), "-o", exe])
    areas = [X.star_area(b"+"), X.star_area(b"-"), EVERY_TYPE + b"XSA-"] + [aux for _, aux, _ in HAND_BUILT if aux]
    out = subprocess.run([exe] + [a.hex() for a in areas], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split()
    assert len(lines) == len(areas)
    for area, line in zip(areas, lines):
        assert [int(line[2 * k:2 * k + 2], 16) for k in range(len(area) + 1)] == [X.py_walk(area[:k]) for k in range(len(area) + 1)]


# ---- the host decoder ----------------------------------------------------------------------------------------------------
NAMES, LENGTHS = ["c1", "c2", "c3"], [10 ** 6] * 3


def _file(tmp_path, tag, seed=5, n=700, **kw):
    rng = np.random.default_rng(seed)
    sets = [(c, X.make_reads(rng, n)) for c in NAMES]
    tags, want = zip(*[X.make_tags(rng, rs) for _, rs in sets])
    path = str(tmp_path / (tag + ".bam"))
    samio.write_bam(path, NAMES, LENGTHS, sets, tags=list(tags), **kw)
    return path, sets, list(tags), list(want)


def _decode(path, threads=2, **kw):
    bam = native.BamFile(path, threads=threads, defer=True, **kw)
    bam.set_aux_strand(True)
    bam.start_host_decode()
    return bam


@pytest.mark.parametrize("kw", [{}, dict(with_seq=True, unplaced=5), dict(long_cigar_tag=True)], ids=["plain", "seq", "cg_tag"])
@pytest.mark.parametrize("threads", [1, 4])
def test_host_decoder_leaves_the_bytes_that_were_written(kw, threads, tmp_path, monkeypatch):
    path, sets, tags, want = _file(tmp_path, "h", **kw)
    for batch in (None, "1"):
        if batch:
            monkeypatch.setenv("SPL_BAM_BATCH_BLOCKS", batch)     # (records straddle the batches: the committing thread's walk extracts them)
        bam = _decode(path, threads)
        for (chrom, rs), t, w in zip(sets, tags, want):
            got = bam.reads(chrom)
            assert np.array_equal(got.pos, rs.pos) and np.array_equal(got.cigar, rs.cigar)
            assert np.array_equal(X.expected_xs(rs, t), w)
            assert got.xs is not None and np.array_equal(got.xs, w), chrom
            assert not got.xs[~X.has_n(rs)].any()          # (0 for a read without an N op, whatever it carries)
            assert {0, PLUS, MINUS} <= set(got.xs.tolist())
        bam.close()


def test_unspliced_reads_that_carry_the_tag_get_no_byte(tmp_path):
    rs = samio.ReadSet.from_records([(0, 10, "50M"), (0, 20, "20M100N30M"), (16, 30, "5S45M"), (0, 40, "10M2D10M90N5M")])
    path = str(tmp_path / "u.bam")
    samio.write_bam(path, ["c"], [10 ** 6], [("c", rs)], tags=[[b"XSA+", b"XSA-", b"XSA-", X.star_area(b"+")]])
    bam = _decode(path, 1)
    assert bam.reads("c").xs.tolist() == [0, MINUS, 0, PLUS]
    bam.close()


def test_without_the_call_there_is_no_fifth_array(tmp_path):
    path, sets, _, _ = _file(tmp_path, "n")
    bam = native.BamFile(path, threads=2)
    for chrom, rs in sets:
        got = bam.reads(chrom)
        assert got.xs is None and np.array_equal(got.pos, rs.pos)
    xp = native.ctypes.c_void_p(1)
    native._check(native.lib().spl_bam_aux_strand(bam._h, 0, native.ctypes.byref(xp)))
    assert not xp.value
    bam.close()


def test_under_a_read_filter_the_bytes_are_the_surviving_reads(tmp_path):
    path, sets, tags, want = _file(tmp_path, "f")
    bam = native.BamFile(path, threads=2, defer=True, exclude_flags=0x110)
    bam.set_aux_strand(True)
    bam.start_host_decode()
    for (chrom, rs), w in zip(sets, want):
        keep = (rs.flag & 0x110) == 0
        got = bam.reads(chrom)
        assert np.array_equal(got.pos, rs.pos[keep]) and np.array_equal(got.xs, w[keep])
    assert bam.filter_counts()[0] == sum(int(((rs.flag & 0x110) != 0).sum()) for _, rs in sets)
    bam.close()


def test_set_aux_strand_is_refused_once_a_decode_has_started(tmp_path):
    path, _, _, _ = _file(tmp_path, "s", n=50)
    bam = native.BamFile(path, threads=1, defer=True)
    bam.set_aux_strand(True)
    bam.set_aux_strand(False)          # (still nobody's: may be changed)
    bam.set_aux_strand(True)
    bam.start_host_decode()
    with pytest.raises(native.SpliserNativeError, match="decoded") as err:
        bam.set_aux_strand(True)
    assert err.value.code == -1      # SPL_ERR_ARG, as from spl_bam_set_filter
    bam.wait_all()
    with pytest.raises(native.SpliserNativeError):
        bam.set_aux_strand(False)
    assert bam.reads("c1").xs is not None
    bam.close()
    for kw in (dict(stream=True), {}):
        bam = native.BamFile(path, threads=1, **kw)
        with pytest.raises(native.SpliserNativeError):
            bam.set_aux_strand(True)
        bam.close()


def test_sam_text_gives_the_same_bytes(tmp_path):
    rng = np.random.default_rng(9)
    rs = X.make_reads(rng, 400)
    text = [("XS:A:+", PLUS), ("NH:i:1\tXS:A:-", MINUS), ("NH:i:1", 0), ("XS:i:37", 0), ("XS:i:37\tXS:A:-", MINUS), ("XS:A:.", 0), ("CO:Z:XS:A:+", 0),
            ("XS:A:+\tXS:A:-", PLUS), ("", 0)]
    binary = [b"XSA+", b"NHC\x01XSA-", b"NHC\x01", b"XSi" + struct.pack("<i", 37), b"XSi" + struct.pack("<i", 37) + b"XSA-", b"XSA.", b"COZXS:A:+\x00",
              b"XSA+XSA-", b""]
    kinds = rng.integers(0, len(text), rs.n)
    sam, bam_path = str(tmp_path / "t.sam"), str(tmp_path / "t.bam")
    with open(sam, "w") as fh:
        fh.write("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c\tLN:1000000\n")
        for k in range(rs.n):
            cols = ["r%d" % k, str(rs.flag[k]), "c", str(rs.pos[k]), "60", samio.cigar_string(rs.cigar[rs.cig_off[k]:rs.cig_off[k + 1]]), "*", "0", "0", "*", "*"]
            fh.write("\t".join(cols + ([text[kinds[k]][0]] if text[kinds[k]][0] else [])) + "\n")
    samio.write_bam(bam_path, ["c"], [10 ** 6], [("c", rs)], tags=[[binary[k] for k in kinds]])
    want = np.where(X.has_n(rs), np.array([text[k][1] for k in kinds]), 0).astype(np.uint8)
    _, sets = samio.read_sam(sam, aux_strand=True)
    assert np.array_equal(sets["c"].xs, want)
    assert samio.read_sam(sam)[1]["c"].xs is None
    bam = _decode(bam_path, 1)
    assert np.array_equal(bam.reads("c").xs, want)
    bam.close()


def test_write_bam_without_tags_writes_what_it_wrote(tmp_path):
    rs = X.make_reads(np.random.default_rng(2), 200)
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    samio.write_bam(a, ["c"], [10 ** 6], [("c", rs)], with_seq=True)
    samio.write_bam(b, ["c"], [10 ** 6], [("c", rs)], with_seq=True, tags=[[b""] * rs.n])
    assert open(a, "rb").read() == open(b, "rb").read()
    with pytest.raises(ValueError):
        samio.write_bam(b, ["c"], [10 ** 6], [("c", rs)], tags=[[b""]])
