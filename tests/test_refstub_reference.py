"""INTEGRATION.md's stub on the reference's own Site objects.  The reference's Steps 0-2 (createGenes, findAlphaCounts,
findCompetitorPos), run unmodified up to the call of ``processSites``, leave a ``site2D_array`` of live Site objects; what those
objects answer through the accessors the stub uses (getPos, getStrand, getAlphaCount, getPartners -- which Site objects, in which
order --, getPartnerCounts, getCompetitorPos) is recorded for every golden case in tests/golden/refstub_live.json.gz.  The test
rebuilds objects that answer exactly that, applies ``refstub.marshal_sites`` to them and has to get, array for array, what this
build's own site table gives for the same files (the arrays every GPU test feeds ``spl_count`` / ``spl_sse`` with).  No GPU, and
no reference needed: the record travels with the tests.  Where the reference is at hand (SPLISER_REFERENCE_DIR), the record is
also held against its live objects, and ``python tests/test_refstub_reference.py --write`` makes it again."""
import gzip
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":     # (run as a script: the package on the path, as conftest.py puts it there for pytest)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import helpers  # noqa: E402
from conftest import golden_cases  # noqa: E402

REF_DIR = os.environ.get("SPLISER_REFERENCE_DIR", "/root/reference")
SCRIPT = os.path.join(REF_DIR, "SpliSER_v0_1_8.py")
HARNESS = os.path.join(helpers.GOLDEN, "..", "..", "oracle", "refharness")
RECORD = os.path.join(helpers.GOLDEN, "refstub_live.json.gz")


def _reference_up_to_step3(case_dir, opts):
    """-> (module, captured processSites arguments): a fresh instance of the reference module after its own process() has run
    Steps 0-2 on the case's files."""
    for p in (os.path.abspath(HARNESS), REF_DIR):      # (the HTSeq stand-in the goldens were made with; the reference's own Site / Gene classes)
        if p not in sys.path:
            sys.path.insert(0, p)
    spec = importlib.util.spec_from_file_location("spliser_reference_under_test", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    argv = sys.argv
    sys.argv = [SCRIPT, "process"]
    try:
        spec.loader.exec_module(mod)
        seen = {}
        mod.processSites = lambda *a, **k: seen.update(args=a, kwargs=k)
        mod.outputBedFile = lambda *a, **k: None
        gff = os.path.join(case_dir, "genes.gff") if opts.get("gff") else None
        mod.process(os.path.join(case_dir, "reads.sam"), os.path.join(case_dir, "junctions.bed"), os.path.join(case_dir, "unused"),
                    opts.get("gene") or "All", opts.get("chrom") or "All", opts.get("max_intron") or 0, gff, "gene",
                    bool(opts.get("stranded")), opts.get("stranded"), bool(opts.get("cryptic")))
    finally:
        sys.argv = argv
    return mod, seen


def _record_of(mod):
    """The reference module's chromosomes and live sites as the stub sees them, in plain data: per site [pos, strand, alpha,
    partners as [row in the chromosome's list or -1, pos], partner counts as [pos, count], competitor positions]."""
    chroms = []
    for sites in mod.site2D_array[:len(mod.chrom_index)]:
        row = {id(s): i for i, s in enumerate(sites)}
        chroms.append([[int(s.getPos()), s.getStrand(), int(s.getAlphaCount(0)),
                        [[row.get(id(p), -1), int(p.getPos())] for p in s.getPartners()],
                        [[int(k), int(v[0])] for k, v in sorted(s.getPartnerCounts().items())],
                        [int(c) for c in s.getCompetitorPos()]] for s in sites])
    return {"chrom_index": list(mod.chrom_index), "sites": chroms}


class _Site(object):
    """A Site as recorded: the accessors marshal_sites calls, answering what the reference's object answered."""

    def __init__(self, pos, strand, alpha):
        self.pos, self.strand, self.alpha = pos, strand, alpha
        self.partners, self.counts, self.competitors = [], {}, []

    def getPos(self): return self.pos
    def getStrand(self): return self.strand
    def getAlphaCount(self, sample): return self.alpha
    def getPartners(self): return self.partners
    def getPartnerCounts(self): return self.counts
    def getCompetitorPos(self): return self.competitors


def _sites_of(recorded):
    sites = [_Site(pos, strand, alpha) for pos, strand, alpha, _, _, _ in recorded]
    for s, (_, _, _, partners, counts, comps) in zip(sites, recorded):
        s.partners = [sites[r] if r >= 0 else _Site(p, "", 0) for r, p in partners]     # (-1: a Site of no row of this list)
        s.counts = {p: [c] for p, c in counts}
        s.competitors = list(comps)
    return sites


def _load_record():
    with gzip.open(RECORD, "rt") as fh:
        return json.load(fh)


def _key(case, variant):
    return "%s/%s" % (case, variant)


@pytest.mark.parametrize("case,variant,opts", golden_cases())
def test_stub_marshalling_on_the_references_live_sites(case, variant, opts, capsys):
    from spliser_amd import refstub
    case_dir = os.path.join(helpers.GOLDEN, case)
    if not os.path.isfile(os.path.join(case_dir, "junctions.bed")):
        pytest.skip("not a process case")
    rec = _load_record()[_key(case, variant)]
    if os.path.isfile(SCRIPT):      # the reference at hand: the record has to be what its live objects answer today
        mod, seen = _reference_up_to_step3(case_dir, opts)
        capsys.readouterr()
        assert seen, "the reference's process() did not reach processSites"
        assert _record_of(mod) == rec, "tests/golden/refstub_live.json.gz is not what the reference's live sites answer"
    table = helpers.build_table(case_dir, opts)
    assert list(rec["chrom_index"]) == list(table.chrom_index)
    n_rows = 0
    for chrom, recorded in zip(rec["chrom_index"], rec["sites"]):
        live = _sites_of(recorded)
        mine = table.chrom_arrays(chrom)
        got = refstub.marshal_sites(live, 0)
        assert len(live) == mine.n
        for name in ("pos", "strand", "part_off", "part_pos", "part_site", "comp_off", "comp_pos", "alpha", "edge_cnt"):
            assert np.array_equal(got[name], np.asarray(getattr(mine, name))), (chrom, name)
        n_rows += len(live)
    assert n_rows > 0


def write_record():
    """Run the reference up to processSites on every golden process case and write what its live sites answer."""
    import contextlib
    import io
    out = {}
    for case, variant, opts in golden_cases():
        case_dir = os.path.join(helpers.GOLDEN, case)
        if not os.path.isfile(os.path.join(case_dir, "junctions.bed")):
            continue
        with contextlib.redirect_stdout(io.StringIO()):
            mod, seen = _reference_up_to_step3(case_dir, opts)
        assert seen, (case, variant)
        out[_key(case, variant)] = _record_of(mod)
    with gzip.GzipFile(RECORD, "wb", mtime=0) as fh:
        fh.write(json.dumps(out, sort_keys=True, separators=(",", ":")).encode("utf-8"))
    return len(out)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_refstub_reference.py --write   (needs the reference: SPLISER_REFERENCE_DIR)")
    print("%d cases written to %s" % (write_record(), RECORD))
