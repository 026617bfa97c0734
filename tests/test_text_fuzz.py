"""The native readers of user-supplied text against the Python they stand in for, on the corpus of textcases.py: about 3 000
files a format, most with byte-level edits, plus file-level edits and one structured case per sentence of the readers' contract.

The contract (csrc/spl_host.cpp, csrc/spl_combine.cpp): whatever a native reader is not sure to read the way Python's str.split /
int() / float() / literal_eval would, it refuses with SPL_ERR_FORMAT, and the caller reads the file in Python.  So for every file
exactly one of two things holds -- the reader refused (-5), or it accepted and says exactly what Python says (and Python did not
raise):

* BED: ``native.read_bed_columns`` against ``_python_bed`` (names, left, right, alpha, strand);
* GFF: ``native.read_gff_genes`` against ``sites.GeneBins.from_annotation`` with ``USE_NATIVE_TEXT`` off (bins, order within a
  bin, names, strand codes, ``n_created``) -- the native entry point itself, not ``from_annotation``, whose ``except Exception``
  would turn a native failure into the Python path;
* .SpliSER.tsv: ``native.Combine`` on [an unharmed file, the corpus file] against ``combine._parse_tsv`` and the Python walk,
  through ``_compare`` of test_combine_native.py (query tables and the bytes of the .combined.tsv), every accepted file in all
  sixteen runs: all genes and one, shallow and not, cryptic and not, stranded and not.

The Python readers are the reference here: the reference-generated goldens pin them (test_text_native.py, test_combine_output.py).

So that nothing passes because everything is refused (or everything is trivial), a format's generated files must be accepted
and refused at a share of 20 % each at least.  Measured with the readers as they are (whole module 34 s on a CPU, no GPU, 32 s of
them the sixteen `combine` runs of each accepted .SpliSER.tsv):
BED 46.7 % accepted / 53.3 % refused, GFF 56.6 % / 43.4 %, .SpliSER.tsv 42.4 % / 57.6 %.

What the corpus found when it was written, each now a structured case of textcases.py: a NUL in a BED or GFF file (the chromosome
"c\\x002" came back as "c", a NUL strand as "no strand"); a byte outside ASCII in a column or line the readers do not look at
(Python raises UnicodeDecodeError on the file, the reader took it) -- both files are refused whole now; and 0x1c-0x1f beside the
first attribute's value of a gene line, which str.strip() takes for blanks (int() does not: int("5\\x1f") is a ValueError, and the
reader refuses that)."""
import os

import pytest

from spliser_amd import native, sites
from test_combine_native import _compare
from test_text_native import _bins_as_lists, _native_bed, _python_bed
import textcases as tc


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return tc.write_corpus(str(tmp_path_factory.mktemp("textcorpus")))


def _refused(call):
    """-> (True, None) when the native reader refused the way the contract allows, (False, its answer) when it accepted."""
    try:
        got = call()
    except native.SpliserNativeError as err:
        assert err.code == -5, "refused with code %d: %s" % (err.code, err)
        return True, None
    return (True, None) if got is None else (False, got)


def _bed(path, work):
    refused, _ = _refused(lambda: native.read_bed_columns(path))
    if refused:
        return False
    assert _native_bed(path) == _python_bed(path)       # (_python_bed raising fails the file: Python raised, native accepted)
    return True


def _gff(path, work):
    refused, cols = _refused(lambda: native.read_gff_genes(path))
    if refused:
        return False
    fast = sites.GeneBins.from_columns(cols)
    sites.USE_NATIVE_TEXT = False
    try:
        slow = sites.GeneBins.from_annotation(path)
    finally:
        sites.USE_NATIVE_TEXT = True
    codes = {c: fast.gene_arrays(c)[2].tolist() for c in fast.chrom_index}      # the column form, before the objects are asked for
    assert _bins_as_lists(fast) == _bins_as_lists(slow)
    assert codes == {c: [43 if g.strand == "+" else (45 if g.strand == "-" else 0) for g in slow.genes[c]] for c in slow.chrom_index}
    return True


def _tsv(path, work, run=None):
    """run: one of textcases.COMBINE_RUNS, or None for all eight (all genes and one, shallow and not, cryptic and not)."""
    good = os.path.join(os.path.dirname(os.path.dirname(path)), "good.SpliSER.tsv")

    def opened():
        with native.Combine([good, path]) as walk:
            return walk.rows(1)
    refused, _ = _refused(opened)
    if refused:
        return False
    for gene, shallow, cryptic in (tc.COMBINE_RUNS if run is None else [tc.COMBINE_RUNS[run]]):
        for stranded in (False, True):
            _compare([good, path], work, stranded, gene, shallow, cryptic)
    return True


CHECK = {"bed": _bed, "gff": _gff, "tsv": _tsv}


def _run(fmt, name, path, work, k=None):
    """-> (accepted, None) or (None, what went wrong, with the file's bytes)."""
    try:
        return (CHECK[fmt](path, work, k) if fmt == "tsv" else CHECK[fmt](path, work)), None
    except Exception as err:        # an assertion above, Python raising on a file the native reader took, or anything else
        with open(path, "rb") as fh:
            return None, "%s %s: %r\n  %s: %s" % (fmt, name, fh.read(), type(err).__name__, str(err)[:400])


@pytest.mark.parametrize("fmt", ["bed", "gff", "tsv"])
def test_generated_files_are_refused_or_read_like_python(fmt, corpus, tmp_path):
    accepted = refused = 0
    failures = []
    for name, path, side in corpus[fmt]:
        took, failure = _run(fmt, name, path, tmp_path)     # (a .SpliSER.tsv the parser takes: all runs of textcases.COMBINE_RUNS)
        if failure:
            failures.append(failure)
        elif name.startswith("g"):
            accepted += 1 if took else 0
            refused += 0 if took else 1
    n = sum(1 for name, _, _ in corpus[fmt] if name.startswith("g"))
    print("%s: %d generated files, %.1f %% accepted, %.1f %% refused, %d failures in the whole corpus"
          % (fmt, n, 100.0 * accepted / n, 100.0 * refused / n, len(failures)))
    assert not failures, "%d files:\n%s" % (len(failures), "\n".join(failures[:20]))
    assert n >= 3000
    assert accepted >= 0.2 * n and refused >= 0.2 * n, (accepted, refused)


def _sided(fmt):
    return [(name, data, side) for name, data, side in
            [("s_" + n, d, s) for n, d, s in tc.STRUCTURED[fmt]] + [("f_" + n, d, s) for n, d, s in tc.file_level(fmt)] if side]


@pytest.mark.parametrize("fmt", ["bed", "gff", "tsv"])
def test_every_structured_case_lands_on_its_side(fmt, corpus, tmp_path):
    paths = {name: path for name, path, _ in corpus[fmt]}
    cases = _sided(fmt)
    assert len(cases) >= 40
    wrong = []
    for name, data, side in cases:
        for run in range(len(tc.COMBINE_RUNS) if fmt == "tsv" else 1):
            took, failure = _run(fmt, name, paths[name], tmp_path, run)
            if failure:
                wrong.append(failure)
            elif took != (side == "accept"):
                wrong.append("%s %s: %r must be %s, was %s" % (fmt, name, data, side + ("ed" if side == "accept" else "d"), "accepted" if took else "refused"))
    assert not wrong, "\n".join(wrong)


def test_a_missing_file_is_an_io_error(tmp_path):
    for call in (native.read_bed_columns, native.read_gff_genes, lambda p: native.Combine([p])):
        with pytest.raises(native.SpliserNativeError) as err:
            call(str(tmp_path / "missing"))
        assert err.value.code == -4
