"""A read set in which no read has a mate, through the per-fragment entry points: ``spl_gene_count_fragments``,
``spl_exon_count_fragments`` and ``spl_coverage_fragments`` give, element for element and special counters included, what
``spl_gene_count``, ``spl_exon_count`` and ``spl_coverage`` give -- and both give what the per-read restatements of ``genecases.py``,
``exoncases.py`` and ``covcases.py`` say.  The four counting kernels share one frame (``CountFrame``) and the three fragment rules
one sides rule (``spl_fragment_sides``); this is where a frame or a rule that went wrong for one of them shows.

The shapes are the smallest at which the frame takes its turns: a set of two segments, one without a read and one of
``2 * TILE + 65`` reads (three workgroups, the last with one full wave, a wave of one lane and two idle waves; a second grid-stride
step needs more than ``GRID_MAX * TILE`` reads and is ``test_a_set_that_gives_every_workgroup_a_second_step``'s, per command);
unstranded with map b empty (null pointers on the device) and stranded with both maps; a map of more entries than the top level
holds (stride 2) and a map of one entry.  The reads carry flags of every kind, paired ones among them, under name keys that are all
distinct: the mate table says "no mate" of every read."""
import os
import re

import numpy as np
import pytest

import covcases as C
import exoncases as X
import genecases as G
from spliser_amd import native, samio

pytestmark = pytest.mark.gpu


def _constant(header, name):
    """A geometry constant of csrc, read from its header."""
    text = open(os.path.join(os.path.dirname(os.path.abspath(native.__file__)), "csrc", header)).read()
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


TILE, TOP = _constant("spl_genecount.h", "SPL_GENE_TILE"), _constant("spl_genecount.h", "SPL_GENE_TOP")
assert (TILE, TOP) == (_constant("spl_exoncount.h", "SPL_EXON_TILE"), _constant("spl_exoncount.h", "SPL_EXON_TOP"))
N_READS, N_MAP = 2 * TILE + 65, TOP + 37
N_GENES, LENGTH = 7, 6400
# (stranded, map a, map b): "big" has N_MAP entries, "one" a single entry
CASES = [(0, "big", None), (1, "big", "one"), (2, "one", "big")]


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def content():
    """The reads, and the maps of both commands: entry k of a big map begins at 60 + 6 k and says nothing, shared, or -- gene map --
    gene (k // 40) % N_GENES, -- bin map -- bin k, whose gene is (k // 40) % N_GENES; a map of one entry says gene 0 / bin 0 from
    base 3000 on."""
    rng = np.random.default_rng(20261023)
    rs = samio.ReadSet.from_records(G.random_records(rng, N_READS, LENGTH + 100))
    assert rs.n == N_READS and int((rs.flag & 1).sum()) > 100
    keys = 2 * np.arange(1, N_READS + 1, dtype=np.uint64)
    start = (60 + 6 * np.arange(N_MAP)).astype(np.int32)
    kind = rng.choice(3, N_MAP, p=[0.25, 0.7, 0.05])
    gene_of = ((np.arange(N_MAP) // 40) % N_GENES).astype(np.uint32)
    code = lambda own: np.where(kind == 0, 0, np.where(kind == 1, own, G.MANY)).astype(np.uint32)
    one = (np.array([3000], np.int32), np.array([1], np.uint32))
    return dict(rs=rs, keys=keys, bin_gene=gene_of, gene={"big": (start, code(gene_of + 1)), "one": one, None: None},
                exon={"big": (start, code(np.arange(1, N_MAP + 1))), "one": one, None: None})


class _Set(object):
    """The reads as the second of two segments of a finished, fused set with name keys; the first segment has no read."""

    def __init__(self, ctx, content):
        self.ctx, self.rs, self.keys = ctx, content["rs"], content["keys"]

    def __enter__(self):
        none = self.rs.take(0, 0)
        arrays = [native.ReadArrays(r.pos, r.flag, r.cig_off, r.cigar, name_key=k) for r, k in ((none, self.keys[:0]), (self.rs, self.keys))]
        self.soa = self.ctx.upload_soa(arrays, with_keys=True)
        self.dr = self.ctx.begin_reads()
        self.dr.add_soa(self.soa, 0)
        self.dr.add_soa(self.soa, 1)
        self.dr.finish()
        assert self.dr.mate_table(0)[1]["paired"] == 0 and self.dr.layout_bytes()[1] == 0          # no read has a mate; the set stays fused
        return self.dr

    def __exit__(self, *exc):
        self.dr.free()
        self.soa.__exit__(*exc)


def _sides(maps, a, b, make):
    """The restatement's view of the call's maps: one (unstranded) or {'+': map a's, '-': map b's}."""
    return make(*maps[a]) if b is None else {"+": make(*maps[a]), "-": make(*maps[b])}


@pytest.mark.parametrize("stranded,a,b", CASES)
def test_gene_counts_per_fragment_are_the_per_read_counts(ctx, content, stranded, a, b):
    maps = content["gene"]
    want = G.counts_of(G.results_of(content["rs"], _sides(maps, a, b, G.bases_of_map), stranded), N_GENES)
    assert sum(want) == N_READS and min(want[N_GENES:]) > 0 and sum(1 for v in want[:N_GENES] if v) >= 5
    with _Set(ctx, content) as dr:
        per_read = dr.gene_counts(N_GENES, maps[a], maps[b], stranded).tolist()
        per_fragment = dr.gene_counts(N_GENES, maps[a], maps[b], stranded, fragments=True).tolist()
    assert per_read == want
    assert per_fragment == want


@pytest.mark.parametrize("stranded,a,b", CASES)
def test_exon_counts_per_fragment_are_the_per_read_counts(ctx, content, stranded, a, b):
    maps, bin_gene = content["exon"], content["bin_gene"]
    labels = _sides(maps, a, b, lambda start, code: X.MapLabels(start, code, bin_gene))
    want = X.counts_of(X.reads_of(content["rs"], labels, stranded), None, N_MAP)
    assert sum(want[N_MAP:]) == N_READS and min(want[N_MAP:]) > 0 and sum(1 for v in want[:N_MAP] if v) >= 50
    with _Set(ctx, content) as dr:
        per_read = dr.exon_counts(bin_gene, maps[a], maps[b], stranded).tolist()
        per_fragment = dr.exon_counts(bin_gene, maps[a], maps[b], stranded, fragments=True).tolist()
    assert per_read == want
    assert per_fragment == want


@pytest.mark.parametrize("stranded,strand", [(0, 0), (1, "+"), (1, "-"), (2, "+")])
def test_coverage_per_fragment_is_the_per_read_coverage(ctx, content, stranded, strand):
    depth, want = C.depth_of(content["rs"], LENGTH, 0, stranded, ord(strand) if strand else 0)
    runs = C.runs_of(depth)
    assert want[1] > 50 and want[2] > 0          # reads contributed, and some lost a base past the end
    with _Set(ctx, content) as dr:
        start, end, run_depth, totals = dr.coverage(LENGTH, stranded, strand)
        f_start, f_end, f_depth, f_totals = dr.coverage(LENGTH, stranded, strand, fragments=True)
    assert C.same_runs((start, end, run_depth), runs) and [totals[k] for k in native.COVERAGE_TOTALS] == [runs[0].shape[0]] + want
    assert C.same_runs((f_start, f_end, f_depth), runs)
    assert [f_totals[k] for k in native.COVERAGE_FRAGMENT_TOTALS] == [runs[0].shape[0]] + want + [0]          # ... and no pair
