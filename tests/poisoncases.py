"""The device paths on poisoned and on reused device memory: the case list and its driver.

Every device buffer of the library comes from the pool of ``spl_capi.cpp`` (``devmem::get``), which hands out dirty memory on purpose.
With ``SPL_DEV_POISON=1`` every buffer is filled with 0xA5 as it is handed out; without it, a process that runs the list a second
time meets buffers that hold the first pass's plausible data.  A case here is a name, a seeded builder of its inputs, a function
that runs it on the device and returns arrays (file texts as bytes), and a yardstick -- the CPU restatements the suites of the
single paths already use.  The driver

    python tests/poisoncases.py --out DIR [--twice] [--only NAME ...] [--list]

runs the list in ONE process, writes each case's raw results to ``DIR/<case>.npz`` and a flushed line ``begin <case>`` /
``end <case>`` to ``DIR/progress.log`` around it, and at the end the pool's statistics and two probes' bytes (``DIR/pool.json``,
``DIR/probes.npz``).  With ``--twice`` it runs the list forward and then once more in reverse order, the second pass under
``DIR/second/``.  It computes no expectation: test_gpu_poisoned_memory.py starts it as a child and compares what it left with
``want_of``; test_poisoncases_host.py checks on the CPU that every yardstick is non-trivial and that ``mismatches`` can fail.

The list: the counting pass at its limits, the BAM decode with every switch and in shares, SAM text and BGZF SAM text, one finished set
under every per-read consumer, the junction table, ``process`` and ``combine`` end to end; and what has been built since the list
was first written, where buffers are reused, regrown and double-buffered inside ONE call: the genome packed at windows of 0, 65536
and 4096 bytes in turn (the same ``DevBuf``s at three sizes; sequences joined inside a 16-byte word the windows share) and under a
store that grows beneath joined sequences (``regrow`` moves what the windows before stored, no more); the motif kernel on one fused
set whose strand bytes all go up wrong, called twice (a tally buffer that is not cleared shows doubled, or as 0xA5), its table and
``spl_junction_motifs``; every ``fragments=True`` consumer on one set with name keys and strand bytes; the text cases again at
``SPL_SAM_WINDOW_BYTES=4096`` -- fifteen windows where the default is one: two text buffers in turn, ``LineIndex`` and the per-line
arrays regrown, the carry of the compressed readers --, plain gzip besides; ``junctions --strandFromMotif`` with text and FASTA in
such windows; and two shards' passes side by side on the two lanes of one context, the mode changing every step."""
import atexit
import hashlib
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import covcases as C                      # noqa: E402
import covfragcases as CF                 # noqa: E402
import exoncases as E                     # noqa: E402
import exonfragcases as EF                # noqa: E402
import filtercases as F                   # noqa: E402
import flagstatcases as fc                # noqa: E402
import genecases as G                     # noqa: E402
import introncases as I                   # noqa: E402
import junctioncases as J                 # noqa: E402
import limitcases as L                    # noqa: E402
import matecases as M                     # noqa: E402
import motifcases as MO                   # noqa: E402
import ordercases as O                    # noqa: E402
import samzcases as Z                     # noqa: E402
import strandcases as S                   # noqa: E402
import windowcases as W                   # noqa: E402
import xscases as X                       # noqa: E402
from spliser_amd import samio             # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
PROBE_BYTES = (3 << 20) + 1               # the pool's granule is 2 MiB: a capacity of 4 MiB
PROBE_SIZES = (1, 2 << 20, (2 << 20) + 1, 5 << 20, (8 << 20) - 1, (20 << 20) + 1)          # further requests, whose capacities are noted
BYTE = {"+": 43, "-": 45, ".": 46}
TRIMS = (0, 30, 49)


class PCase(object):
    """name; build(workdir) -> inputs (a dict; files it needs are written under workdir); run(ctx, inputs, outdir) -> {key: array
    or bytes}, on the device; want(inputs) -> the same keys from the yardstick; nontrivial(inputs, want): asserts, on the CPU, that
    the yardstick is worth comparing with."""

    def __init__(self, name, build, run, want, nontrivial):
        self.name, self.build, self.run, self.want, self.nontrivial = name, build, run, want, nontrivial


def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


def _env(**kv):
    """Context manager: environment variables for the span of one run, put back after it."""
    class _E(object):
        def __enter__(self):
            self.old = {k: os.environ.get(k) for k in kv}
            os.environ.update({k: str(v) for k, v in kv.items()})

        def __exit__(self, *exc):
            for k, v in self.old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return _E()


def _arrays(features):
    return (np.array([f[0] for f in features], np.int64), np.array([f[1] for f in features], np.int64), np.array([BYTE[f[2]] for f in features], np.uint8),
            np.array([f[3] for f in features], np.int64))


def _tables(introns):
    off = np.zeros(len(introns) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in introns])
    return off, np.array([p[0] for pieces in introns for p in pieces], np.int32), np.array([p[1] for pieces in introns for p in pieces], np.int32)


def _text(a):
    """A file's text back from the bytes it is kept as."""
    return np.asarray(a, np.uint8).tobytes().decode("latin-1")


def _rows(rows):
    return np.asarray(rows, np.int64).reshape(-1, 6)


# ---- count: limitcases.count_device -------------------------------------------------------------------------------------------
COUNT_CASES = [
    ("non_consuming_ops", lambda: {c.name: c for c in L.parity_cases()}["non_consuming_ops"]),
    ("twice_spliced_class_limits", lambda: {c.name: c for c in L.parity_cases()}["twice_spliced_class_limits"]),
    ("more_ops_than_the_packed_count", lambda: {c.name: c for c in L.parity_cases()}["more_ops_than_the_packed_count"]),
    ("window_%d" % L.WIN, lambda: L.window_case(L.WIN)),
    ("rivals_once_%d" % (L.RIV_ONCE + 1), lambda: L.rival_case("once_%d" % (L.RIV_ONCE + 1))),
    ("overflow_front_first", lambda: L.overflow_case("front_first")),
    ("tile_class_change_%d" % (L.TILE + 1), lambda: L.tile_case("class_change_%d" % (L.TILE + 1))),
    ("scan_%d" % (L.SCAN_BLOCK + 1), lambda: L.scan_case(L.SCAN_BLOCK + 1)),
]
SECOND_MODES = [(1, 0), (2, 1), (1, 1), (2, 0)]          # a case's one stranded / combine mode, dealt out in turn


def _count_runs(inp):
    """(chunk, fused, stranded, combine) of a count case's runs, and the tag of each in the results."""
    for chunk in inp["chunks"]:
        for fused in (0, 1):
            for stranded, combine in inp["modes"]:
                yield chunk, fused, stranded, combine, "chunk%d_fused%d_s%d_c%d_" % (chunk, fused, stranded, combine)


def _count_case(k, name, make):
    modes = [(0, 0), SECOND_MODES[k % len(SECOND_MODES)]]
    # every case at SPL_FORCE_CHUNK = CHUNK; the overflow case at CHUNK_BIG too, where the fused pass's lists run full and their
    # entries go straight to the literal queue (at CHUNK the queue holds its flag-0x4 reads only)
    chunks = [L.CHUNK, L.CHUNK_BIG] if name.startswith("overflow_") else [L.CHUNK]

    def build(workdir):
        return dict(case=make(), modes=modes, chunks=chunks)

    def run(ctx, inp, outdir):
        case, out = inp["case"], {}
        sites = case.table.sites()
        for chunk, fused, stranded, combine, tag in _count_runs(inp):
            with _env(SPL_FORCE_CHUNK=chunk, SPL_FUSED=fused):
                got = L.count_device(ctx, sites, case.segments, stranded, combine, (stranded + combine) % 2 == 0)
            for j, a in enumerate(got.counters):
                out[tag + "counter%d" % j] = np.asarray(a)
            for j, a in enumerate(got.sse):
                out[tag + "sse%d" % j] = np.asarray(a)
            out[tag + "stayed_fused"] = np.array([int(got.fused)])
            if name.startswith("overflow_") and not combine:
                out[tag + "queued"] = np.array([got.queued])
        return out

    def want(inp):
        oracle, case, out = _oracle(), inp["case"], {}
        t, r = case.table, case.reads
        memo = {}
        for chunk, fused, stranded, combine, tag in _count_runs(inp):
            if (stranded, combine) not in memo:
                counts = oracle.check_bam(t.pos, t.strand, t.part_off, t.part_pos, t.comp_off, t.comp_pos, r.pos, r.flag, r.cig_off, r.cigar, stranded, combine)
                sse = oracle.beta2_sse(t.pos, t.part_off, t.part_pos, t.part_site, t.alpha, t.edge_cnt, counts[0], counts[1], counts[2], (stranded + combine) % 2 == 0)
                memo[(stranded, combine)] = (counts, sse)
            counts, sse = memo[(stranded, combine)]
            for j, a in enumerate(counts):
                out[tag + "counter%d" % j] = np.asarray(a)
            for j, a in enumerate(sse):
                out[tag + "sse%d" % j] = np.asarray(a)
            out[tag + "stayed_fused"] = np.array([fused])
            if name.startswith("overflow_") and not combine:          # the flag-0x4 reads, and the list entries that did not fit
                out[tag + "queued"] = np.array([case.meta["n_literal"] + L.simulate_lists(case, bool(fused), chunk)[1]])
        return out

    def nontrivial(inp, w):
        case = inp["case"]
        for stranded, combine in inp["modes"]:
            b1, b2 = w["chunk%d_fused1_s%d_c%d_counter0" % (L.CHUNK, stranded, combine)], w["chunk%d_fused1_s%d_c%d_counter1" % (L.CHUNK, stranded, combine)]
            # (overflow: nothing but spliced reads with rivals, no beta1; the 70 000-op case: four reads, one junction, no rival)
            assert int(b1.sum()) > 0 or name.startswith("overflow_"), (name, stranded, combine)
            assert int(b2.sum()) > 0 or name.startswith("more_ops_"), (name, stranded, combine)
        assert case.reads.n > 0 and case.table.n > 0
        if name.startswith("scan_"):
            assert len(case.table.dpos()) == L.SCAN_BLOCK + 1 > L.SCAN_BLOCK          # boundaries above one scan tile
        if name.startswith("tile_"):
            assert case.reads.n > L.CHUNK and case.reads.n > L.TILE                   # more than one chunk, more than one tile
        if name.startswith("overflow_"):
            assert w["chunk%d_fused1_s0_c0_queued" % L.CHUNK][0] == case.meta["n_literal"] > 0          # the literal queue is used ...
            assert w["chunk%d_fused1_s0_c0_queued" % L.CHUNK_BIG][0] > case.meta["n_literal"]           # ... and takes what full lists hand over
        if name.startswith("rivals_"):
            assert case.meta["n_rivals"] == L.RIV_ONCE + 1
        if name.startswith("window_"):
            assert case.table.n > L.WIN

    return PCase("count_" + name, build, run, want, nontrivial)


# ---- decode: the file of test_decode_all_options --------------------------------------------------------------------------------
DEC_NAMES = ["a", "b", "c"]
DEC_FILT = (10, 0, 0x400)
DEC_BLOCK = 4096
DEC_ALL = dict(min_mapq=DEC_FILT[0], require_flags=DEC_FILT[1], exclude_flags=DEC_FILT[2], aux_strand=True, flagstat=True, any_order=True)


def _decode_build(workdir):
    d = os.path.join(workdir, "decode")
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(20261018)
    sets, tags, mapq = [], [], []
    for _ in DEC_NAMES:
        rs = X.make_reads(rng, 1500)
        flag = np.asarray(rs.flag, np.int64) | np.where(rng.random(rs.n) < 0.07, 0x400, 0)
        sets.append(samio.ReadSet(rs.pos, flag, rs.cig_off, rs.cigar))
        tags.append(X.make_tags(rng, rs)[0])
        mapq.append(rng.integers(0, 61, rs.n))
    unplaced = [(-1, 0, 0x4, 0, [], b""), (-1, 0, 0x4 | 0x200, 255, [], b""), (-1, 0, 0x4 | 0x1 | 0x8 | 0x40, 30, [], b"")]
    in_order = O.records_of(sets, tags=tags, mapq=mapq) + unplaced
    mixed = O.shuffled(in_order, 7)
    sorted_path, shuffled_path = os.path.join(d, "sorted.bam"), os.path.join(d, "shuffled.bam")
    O.write_bam(sorted_path, DEC_NAMES, [10 ** 6] * 3, in_order, so="coordinate", block=DEC_BLOCK)
    O.write_bam(shuffled_path, DEC_NAMES, [10 ** 6] * 3, mixed, so="unsorted", block=DEC_BLOCK)
    return dict(in_order=in_order, mixed=mixed, sorted_path=sorted_path, shuffled_path=shuffled_path)


def _decoded(bam, out, with_keys):
    for name in DEC_NAMES:
        got = bam.reads(name)
        for k in ("pos", "flag", "cig_off", "cigar", "xs") + (("name_key",) if with_keys else ()):
            out["%s_%s" % (name, k)] = np.asarray(getattr(got, k))
    out["filter_counts"] = np.asarray(bam.filter_counts(), np.int64)
    out["n_records"] = np.array([bam.n_records], np.int64)
    out["flagstat"] = np.asarray(bam.flagstat())
    n, by_device = bam.any_order_sorted()
    out["any_order_sorted"] = np.array([n, int(by_device)], np.int64)


def _decode_want(inp, records, with_keys, sorted_by_device):
    want = O.expected(records, len(DEC_NAMES), DEC_FILT)
    out = {}
    for t, name in enumerate(DEC_NAMES):
        rs, tags = want[t]
        out[name + "_pos"], out[name + "_flag"], out[name + "_cig_off"], out[name + "_cigar"] = rs.pos, rs.flag, rs.cig_off, rs.cigar
        out[name + "_xs"] = X.expected_xs(rs, tags)
        if with_keys:
            out[name + "_name_key"] = np.full(rs.n, M.name_key(b"r"), np.uint64)          # (ordercases.record names every read "r")
    tid, pos, flag, q = (np.array([r[k] for r in inp["in_order"]], np.int64) for k in range(4))
    placed = (tid >= 0) & (pos >= 1)
    kept, by_flags, by_mapq = F.keep_mask(flag, q, DEC_FILT)
    out["filter_counts"] = np.array([int((by_flags & placed).sum()), int((by_mapq & placed).sum())], np.int64)
    out["n_records"] = np.array([len(inp["in_order"])], np.int64)
    out["flagstat"] = fc.restate_filtered(flag, tid, np.full(len(tid), -1), q, DEC_FILT)
    out["any_order_sorted"] = np.array([int((kept & placed).sum()), 1] if sorted_by_device else [0, 0], np.int64)
    return out


def _decode_nontrivial(inp, w):
    assert min(w["filter_counts"].tolist()) > 0                                      # a dropped read in each filter class
    assert all(w[n + "_pos"].shape[0] > 1000 for n in DEC_NAMES) and all(int(np.count_nonzero(w[n + "_xs"])) > 100 for n in DEC_NAMES)
    assert int(w["flagstat"][2].sum()) > 0 and int(w["flagstat"][4].sum()) == 0 and int(w["flagstat"][:, 1].sum()) > 0          # secondary; no duplicate left; QC-failed
    assert os.path.getsize(inp["shuffled_path"]) > 40 * 1000                         # some eighty blocks: many windows of two


def _decode_shuffled_run(ctx, inp, outdir):
    from spliser_amd import native
    out = {}
    with _env(SPL_INFLATE_WINDOW_BLOCKS=2):
        bam = native.BamFile(inp["shuffled_path"], threads=2, defer=True, mate_keys=True, **DEC_ALL)
        try:
            if bam.decode_on_device(ctx) is not True:
                raise RuntimeError("the device decode declined: %s" % bam.decline_reason())
            if bam.wait_all() is not True:
                raise RuntimeError("wait_all")
            _decoded(bam, out, True)
        finally:
            bam.close()
    return out


def _decode_shares_run(ctx, inp, outdir):
    from spliser_amd import native
    out = {}
    bam = native.BamFile(inp["sorted_path"], threads=2, defer=True, **dict(DEC_ALL, any_order=False))
    try:
        out["n_shares"] = np.array([len(bam.decode_on_devices_async([0, 0, 0]))])
        if bam.join_decoders() is not True:
            raise RuntimeError("the decode in shares declined: %s" % bam.decline_reason())
        _decoded(bam, out, False)
    finally:
        bam.close()
    return out


def _decode_shares_want(inp):
    out = _decode_want(inp, inp["in_order"], False, False)
    out["n_shares"] = np.array([3])
    return out


# ---- text: test_gpu_fragments' generated pairs as SAM and BGZF SAM ----------------------------------------------------------------
TXT_NAMES, TXT_LENGTHS = ["c1", "c2"], [10 ** 6] * 2
TXT_IDS = ["gene%02d" % k for k in range(8)]
TXT_SPAN = 20000
TXT_FRAGMENTS = 300


def _text_build(workdir):
    d = os.path.join(workdir, "text")
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(41)
    sets, names, mapq, features = [], [], [], {}
    for k, chrom in enumerate(TXT_NAMES):
        records, nm, _ = M.paired_records(rng, TXT_FRAGMENTS, TXT_SPAN)
        keep = [j for j, r in enumerate(records) if r[1] >= 1]          # (a file has no POS 0 on a reference)
        records, nm = [records[j] for j in keep], [nm[j] for j in keep]
        records += [(99, TXT_SPAN + 45, "20M"), ((99, 147)[k], TXT_SPAN + 50, "30M"), (147, TXT_SPAN + 90, "30M")]
        nm += [b"lowq%d" % k, b"split/pair", b"lowq%d" % k]
        sets.append((chrom, samio.ReadSet.from_records(records)))
        names.append(nm)
        q = np.full(len(records), 60, np.int64)
        q[-1] = 3
        mapq.append(q)
        features[chrom] = [(l, r, s, g) for l, r, s, g in G.random_features(rng, TXT_SPAN, 8, 40)] + [(TXT_SPAN + 40, TXT_SPAN + 70, "+", k), (TXT_SPAN + 85, TXT_SPAN + 130, "+", 2 + k)]
    sam, samz, gtf = os.path.join(d, "p.sam"), os.path.join(d, "p.sam.gz"), os.path.join(d, "genes.gtf")
    samio.write_sam(sam, TXT_NAMES, TXT_LENGTHS, sets, names=names, mapq=mapq)
    with open(sam, "rb") as fh, open(samz, "wb") as out:
        out.write(Z.bgzf(fh.read(), block=0xff00))
    text = "##gtf of the tests\n"
    for chrom in TXT_NAMES:
        for j, (left, right, strand, gene) in enumerate(features[chrom]):
            text += "%s\tsynth\texon\t%d\t%d\t.\t%s\t.\tgene_id \"%s\"; transcript_id \"t%d\";\n" % (chrom, left + 1, right, strand, TXT_IDS[gene], j)
    with open(gtf, "w") as fh:
        fh.write(text)
    ids, by_chrom = G.features_of_text(text)
    assert ids == TXT_IDS
    keys = [np.array([M.name_key(n) for n in nm], np.uint64) for nm in names]
    return dict(sam=sam, samz=samz, gtf=gtf, sets=sets, keys=keys, by_chrom=by_chrom)


def _fragments_run(which):
    def run(ctx, inp, outdir):
        from spliser_amd import cli, process as proc
        prefix = os.path.join(outdir, "fragments_" + which)
        if cli.main(["genecounts", "-A", inp["gtf"], "-o", prefix, "--fragments", "-B", inp[which]]) != 0:
            raise RuntimeError("genecounts --fragments failed")
        proc.wait_deferred_close()
        return {"genecounts.tsv": open(prefix + ".genecounts.tsv", "rb").read()}
    return run


def _fragments_counts(inp):
    out, pairs = [0] * (len(TXT_IDS) + 3), 0
    for (chrom, rs), keys in zip(inp["sets"], inp["keys"]):
        feats = inp["by_chrom"].get(chrom, [])
        bases = G.bases_of_features(feats, TXT_SPAN + 2100)
        mate, counts = M.mate_table_of(rs, keys)
        pairs += counts["paired"] // 2
        got = M.counts_of(M.fragment_results(rs, keys, bases, 0, mate=mate), len(TXT_IDS))
        out = [x + y for x, y in zip(out, got)]
    return out, pairs


def _fragments_want(inp):
    return {"genecounts.tsv": G.file_text(TXT_IDS, _fragments_counts(inp)[0]).encode()}


def _fragments_nontrivial(inp, w):
    counts, pairs = _fragments_counts(inp)
    assert pairs > 300 and sum(counts) == sum(rs.n for _, rs in inp["sets"]) - pairs          # pairs above zero: a fragment counts once
    assert min(counts[len(TXT_IDS):]) > 0 and sum(1 for c in counts[:len(TXT_IDS)] if c) >= 5        # every special counter above zero
    assert os.path.getsize(inp["samz"]) < os.path.getsize(inp["sam"])


def _text_coverage_run(ctx, inp, outdir):
    from spliser_amd import cli, process as proc
    prefix = os.path.join(outdir, "coverage_sam")
    if cli.main(["coverage", "-B", inp["sam"], "-o", prefix]) != 0:
        raise RuntimeError("coverage failed")
    proc.wait_deferred_close()
    return {"bedgraph": open(prefix + ".bedgraph", "rb").read()}


def _text_coverage_want(inp):
    text = ""
    for (chrom, rs), ln in zip(inp["sets"], TXT_LENGTHS):
        depth, _ = C.depth_of(rs, ln)
        text += C.bedgraph_text(chrom, *C.runs_of(depth))
    return {"bedgraph": text.encode()}


def _text_coverage_nontrivial(inp, w):
    lines = _text(w["bedgraph"]).splitlines()
    assert len(lines) > 500 and {ln.split("\t")[0] for ln in lines} == set(TXT_NAMES) and any(int(ln.split("\t")[3]) > 2 for ln in lines)


# ---- one finished set, every consumer in turn ---------------------------------------------------------------------------------
SET_LENGTH = 149000
SET_BASES = 160000                     # (the reads run past SET_LENGTH: the per-base yardsticks of the counts look this far)
SET_GENES = 9


def _oneset_build(workdir):
    rng = np.random.default_rng(20261020)
    rs = X.make_reads(rng, 3000, long_cigar_every=97)
    _, xs = X.make_tags(rng, rs)
    names = M.paired_records(rng, 1400, SET_LENGTH)[1]
    assert len(names) >= rs.n
    keys = np.array([M.name_key(n) for n in names[:rs.n]], np.uint64)
    features = G.random_features(rng, SET_LENGTH - 1000, SET_GENES, 30)
    start = np.sort(rng.choice(np.arange(1, SET_LENGTH), 1000, replace=False)).astype(np.int32)
    cover = (start, rng.integers(0, 4, 1000).astype(np.uint8))
    return dict(rs=rs, xs=xs, keys=keys, features=features, cover=cover)


def _oneset_run(ctx, inp, outdir):
    from spliser_amd import exoncounts as xc, genecounts as gc, native
    rs, xs, keys, features = inp["rs"], inp["xs"], inp["keys"], inp["features"]
    out, records_bytes = {}, []
    a, _ = gc.gene_maps(*_arrays(features))
    plus, minus = gc.gene_maps(*_arrays(features), stranded=True)
    bin_map, _, (bin_gene, _, _) = xc.exon_maps(*_arrays(features), stranded=False)
    introns = [x[3] for x in I.introns_of(features, ".", SET_LENGTH)]

    def coverage(tag, *args):
        start, end, depth, t = dr.coverage(SET_LENGTH, *args)
        out[tag + "_start"], out[tag + "_end"], out[tag + "_depth"] = start, end, depth
        out[tag + "_totals"] = np.array([t["reads_seen"], t["contributed"], t["past_end"], t["covered_bases"], t["runs"]], np.int64)

    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, xs=xs, name_key=keys)], with_strand=True, with_keys=True) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            records_bytes.append(dr.layout_bytes()[1])
            out["strand_tally"] = dr.strand_tally(inp["cover"]); records_bytes.append(dr.layout_bytes()[1])
            coverage("coverage"); records_bytes.append(dr.layout_bytes()[1])
            coverage("coverage_fr_plus", 1, "+"); records_bytes.append(dr.layout_bytes()[1])
            out["gene_counts"] = dr.gene_counts(SET_GENES, a); records_bytes.append(dr.layout_bytes()[1])
            out["gene_counts_fr"] = dr.gene_counts(SET_GENES, plus, minus, 1); records_bytes.append(dr.layout_bytes()[1])
            out["gene_counts_fragments"] = dr.gene_counts(SET_GENES, a, fragments=True); records_bytes.append(dr.layout_bytes()[1])
            mate, counts = dr.mate_table(0, rs.n); records_bytes.append(dr.layout_bytes()[1])
            out["mate"], out["mate_counts"] = mate, np.array([counts[k] for k in native.MATE_COUNTS], np.int64)
            out["exon_counts"] = dr.exon_counts(bin_gene.astype(np.uint32), bin_map); records_bytes.append(dr.layout_bytes()[1])
            out["intron_depth_of_the_set"] = dr.intron_depth(SET_LENGTH, *_tables(introns), trim_percent=30); records_bytes.append(dr.layout_bytes()[1])
            for k, (_, pos, depth, pieces, length) in enumerate(I.body_cases()):
                for trim in TRIMS:
                    out["intron_body%02d_trim%d" % (k, trim)] = native.intron_depth_runs(ctx, pos, depth, length, *_tables(pieces), trim_percent=trim)
            records_bytes.append(dr.layout_bytes()[1])
            out["junctions"] = _rows(J.rows(dr.junctions(0))); records_bytes.append(dr.layout_bytes()[1])
            out["junctions_from_xs"] = _rows(J.rows(dr.junctions(native.STRAND_FROM_XS))); records_bytes.append(dr.layout_bytes()[1])
            coverage("coverage_again"); records_bytes.append(dr.layout_bytes()[1])
    out["record_bytes_after_every_call"] = np.asarray(records_bytes, np.int64)
    return out


def _oneset_want(inp):
    from spliser_amd import exoncounts as xc
    oracle = _oracle()
    rs, xs, keys, features = inp["rs"], inp["xs"], inp["keys"], inp["features"]
    out = {"strand_tally": np.asarray(S.tally(rs, xs, inp["cover"]), np.int64)}
    for tag, args in (("coverage", ()), ("coverage_fr_plus", (1, "+"))):
        depth, totals = C.depth_of(rs, SET_LENGTH, 0, *args)
        start, end, value = C.runs_of(depth)
        out[tag + "_start"], out[tag + "_end"], out[tag + "_depth"] = start, end, value
        out[tag + "_totals"] = np.array(totals + [start.shape[0]], np.int64)
        if tag == "coverage":
            per_base = depth
    for k in ("start", "end", "depth", "totals"):
        out["coverage_again_" + k] = out["coverage_" + k]
    bases = G.bases_of_features(features, SET_BASES)
    both = {w: G.bases_of_features(features, SET_BASES, w) for w in "+-"}
    out["gene_counts"] = np.asarray(G.counts_of(G.results_of(rs, bases), SET_GENES), np.int64)
    out["gene_counts_fr"] = np.asarray(G.counts_of(G.results_of(rs, both, 1), SET_GENES), np.int64)
    mate, counts = M.mate_table_of(rs, keys)
    out["gene_counts_fragments"] = np.asarray(M.counts_of(M.fragment_results(rs, keys, bases, mate=mate), SET_GENES), np.int64)
    out["mate"] = np.asarray(mate, np.int64)
    out["mate_counts"] = np.array([counts[k] for k in ("pairable", "paired", "unpaired_mate_mapped")], np.int64)
    labels = E.labels_of_features(features, SET_BASES)
    bins = E.bins_of([labels])
    _, _, (bin_gene, bin_start, bin_end) = xc.exon_maps(*_arrays(features), stranded=False)
    assert list(zip(bin_start.tolist(), bin_end.tolist(), bin_gene.tolist())) == bins          # (the product's bins are the yardstick's)
    out["exon_counts"] = np.asarray(E.counts_of(E.reads_of(rs, labels), {k: i for i, k in enumerate(bins)}, len(bins)), np.int64)
    introns = [x[3] for x in I.introns_of(features, ".", SET_LENGTH)]
    out["intron_depth_of_the_set"] = np.asarray([I.stats_of(per_base, pieces, 30) for pieces in introns], np.int64).reshape(-1, 4)
    for k, (_, pos, depth, pieces, length) in enumerate(I.body_cases()):
        per = I.depth_per_base(pos, depth, length)
        for trim in TRIMS:
            out["intron_body%02d_trim%d" % (k, trim)] = np.asarray([I.stats_of(per, p, trim) for p in pieces], np.int64).reshape(-1, 4)
    out["junctions"] = _rows(oracle.junction_table(rs.pos, rs.flag, rs.cig_off, rs.cigar, 0, 0, 0, 0))
    out["junctions_from_xs"] = _rows(X.yardstick(rs, xs))
    out["record_bytes_after_every_call"] = np.zeros(14, np.int64)          # the set stays fused: no records are ever written
    return out


def _oneset_nontrivial(inp, w):
    assert min(w["strand_tally"].tolist()) > 0
    assert w["coverage_start"].shape[0] > L.SCAN_BLOCK and w["coverage_totals"][2] > 0          # boundaries above one scan tile; reads past the end
    assert 0 < w["coverage_fr_plus_totals"][1] < w["coverage_totals"][1]
    for k in ("gene_counts", "gene_counts_fr", "gene_counts_fragments"):
        assert min(w[k][SET_GENES:].tolist()) > 0 and sum(1 for c in w[k][:SET_GENES] if c) >= 5, k          # every special counter above zero
    assert w["mate_counts"][1] >= 40 and not np.array_equal(w["gene_counts"], w["gene_counts_fragments"])     # pairs above zero
    assert int(w["gene_counts_fragments"].sum()) == inp["rs"].n - w["mate_counts"][1] // 2
    n_bins = w["exon_counts"].shape[0] - 4
    assert min(w["exon_counts"][n_bins:].tolist()) > 0 and int(np.count_nonzero(w["exon_counts"][:n_bins])) > 10
    assert w["intron_depth_of_the_set"].shape[0] > 3 and int(w["intron_depth_of_the_set"][:, 1].sum()) > 0
    assert w["junctions"].shape[0] >= 30 and {43, 45, 63} <= set(w["junctions_from_xs"][:, 2].tolist())
    assert int(np.diff(inp["rs"].cig_off.astype(np.int64)).max()) > 80                                       # the long CIGARs are there


# ---- junctions: junctioncases against oracle.junction_table -----------------------------------------------------------------------
def _junction_case(name):
    def build(workdir):
        return dict(case=J.case(name))

    def run(ctx, inp, outdir):
        from spliser_amd import native
        case, out = inp["case"], {}
        for fused in (0, 1):
            with _env(SPL_FORCE_CHUNK=J.CHUNK, SPL_FUSED=fused):
                with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar) for rs, _ in case.segments]) as soa:
                    with ctx.begin_reads() as dr:
                        for k, (_, shift) in enumerate(case.segments):
                            dr.add_soa(soa, k, shift)
                        dr.finish()
                        for stranded in (0, 1, 2):
                            for a, m, mx in case.filters:
                                out["fused%d_s%d_a%d_m%d_M%d" % (fused, stranded, a, m, mx)] = _rows(J.rows(dr.junctions(stranded, a, m, mx)))
                        out["fused%d_stayed_fused" % fused] = np.array([int(dr.layout_bytes()[1] == 0)])
        return out

    def want(inp):
        case, out = inp["case"], {}
        for stranded in (0, 1, 2):
            for a, m, mx in case.filters:
                rows = _rows(case.want(stranded, a, m, mx))
                for fused in (0, 1):
                    out["fused%d_s%d_a%d_m%d_M%d" % (fused, stranded, a, m, mx)] = rows
        for fused in (0, 1):
            out["fused%d_stayed_fused" % fused] = np.array([fused])
        return out

    def nontrivial(inp, w):
        a, m, mx = inp["case"].filters[0]
        for stranded in (0, 1, 2):
            t = w["fused1_s%d_a%d_m%d_M%d" % (stranded, a, m, mx)]
            assert t.shape[0] > 3 and int(t[:, 3].sum()) > t.shape[0], (name, stranded)          # junctions, and counts above one
        assert {43, 45} <= set(w["fused1_s1_a%d_m%d_M%d" % (a, m, mx)][:, 2].tolist())

    return PCase("junctions_" + name, build, run, want, nontrivial)


# ---- end to end: the goldens the real reference wrote ---------------------------------------------------------------------------
KAT2 = os.path.join(GOLDEN, "kat2")
# kat2's junctions.bed holds three of the four junctions of its reads -- the fourth has anchors of ten bases -- with the strands an
# fr library gives them: `process` without -b finds exactly those under --minAnchor 11, stranded fr.
KAT2_FLAGS = ["--isStranded", "-s", "fr", "--minAnchor", "11", "--keepReads", "--flagstat"]
COMBINE = os.path.join(GOLDEN, "combine_a")
COMBINE_VARIANT = "fr_cryptic"


def _kat2_run(ctx, inp, outdir):
    from spliser_amd import cli, flagstat as fstat, process as proc
    prefix = os.path.join(outdir, "kat2")
    if cli.main(["process", "-B", os.path.join(KAT2, "reads.sam"), "-o", prefix] + KAT2_FLAGS) != 0:
        raise RuntimeError("process failed")
    proc.wait_deferred_close()
    return {"SpliSER.tsv": open(prefix + ".SpliSER.tsv", "rb").read(), "flagstat.txt": open(prefix + fstat.SUFFIX, "rb").read()}


def _kat2_want(inp):
    from spliser_amd import flagstat as fstat
    flag, mapq, next_tid = [], [], []
    for line in open(os.path.join(KAT2, "reads.sam")):
        if not line.startswith("@"):
            col = line.split("\t")
            flag.append(int(col[1])); mapq.append(int(col[4])); next_tid.append(0 if col[6] == "=" else -1)
    counts = fc.restate(np.array(flag), np.zeros(len(flag), np.int64), np.array(next_tid), np.array(mapq))
    return {"SpliSER.tsv": open(os.path.join(KAT2, "expected.fr.tsv"), "rb").read(), "flagstat.txt": ("\n".join(fstat.format_lines(counts)) + "\n").encode()}


def _kat2_nontrivial(inp, w):
    lines = _text(w["SpliSER.tsv"]).splitlines()
    assert len(lines) == 6 and any(int(ln.split("\t")[6]) > 0 for ln in lines[1:]) and any(int(ln.split("\t")[7]) > 0 for ln in lines[1:])
    assert _text(w["flagstat.txt"]).startswith("11 + 0 in total")


def _combine_run(ctx, inp, outdir):
    from spliser_amd import cli, process as proc
    manifest = json.load(open(os.path.join(COMBINE, "combine_manifest.json")))
    sfile = os.path.join(outdir, "samples.tsv")
    with open(sfile, "w") as fh:
        for k in range(manifest["n_samples"]):
            sd = os.path.join(COMBINE, "sample%d" % k)
            fh.write("S%d\t%s\t%s\n" % (k, os.path.join(sd, "expected.%s.tsv" % COMBINE_VARIANT), os.path.join(sd, "reads.sam")))
    v = manifest["variants"][COMBINE_VARIANT]
    if cli.main([v.get("command", "combine"), "-S", sfile, "-o", os.path.join(outdir, "all")] + v["combine"]) != 0:
        raise RuntimeError("combine failed")
    proc.wait_deferred_close()
    return {"combined.tsv": open(os.path.join(outdir, "all.combined.tsv"), "rb").read()}


def _combine_want(inp):
    return {"combined.tsv": open(os.path.join(COMBINE, "expected.%s.combined.tsv" % COMBINE_VARIANT), "rb").read()}


def _combine_nontrivial(inp, w):
    lines = _text(w["combined.tsv"]).splitlines()
    assert len(lines) > 20 and len(lines[0].split("\t")) > 6


# ---- the genome on the device: one set of buffers at three window sizes, and a store that grows under joined sequences ----------------
GENOME_WINDOWS = (0, 65536, 4096)          # in this order, in one process: the same DevBufs are asked for three different sizes


def _genome_pack_build(workdir):
    os.makedirs(workdir, exist_ok=True)
    path = os.path.join(workdir, "corpus.fa")
    with open(path, "wb") as fh:
        fh.write(MO.pack_corpus())
    return dict(path=path)


def _genome_pack_run(ctx, inp, outdir):
    from spliser_amd import native
    out = {}
    for window in GENOME_WINDOWS:
        tag = "window%d_" % window
        with native.Genome(ctx, inp["path"], window) as g:
            out[tag + "names"] = "\n".join(g.names).encode("utf-8", "surrogateescape")
            out[tag + "lengths"] = np.asarray(g.lengths, np.int64)
            out[tag + "bases"] = np.concatenate([g.bases(k) for k in range(len(g.names))])
            out[tag + "device_bytes"] = np.array([g.stats()["device_bytes"]], np.int64)
    return out


def _genome_pack_want(inp):
    seqs = MO.parse_fasta(open(inp["path"], "rb").read())
    out = {}
    for window in GENOME_WINDOWS:
        tag = "window%d_" % window
        out[tag + "names"] = b"\n".join(n for n, _ in seqs)
        out[tag + "lengths"] = np.array([len(c) for _, c in seqs], np.int64)
        out[tag + "bases"] = np.concatenate([c for _, c in seqs])
        out[tag + "device_bytes"] = np.array([sum(16 * ((len(c) + 31) // 32) for _, c in seqs)], np.int64)
    return out


def _genome_pack_nontrivial(inp, w):
    text = open(inp["path"], "rb").read()
    assert len(text) == 559453 and w["window0_lengths"].shape[0] == 71 and int(np.count_nonzero(w["window0_lengths"] == 0)) >= 1
    joined = MO.sequences_joined_across(text, 4096)
    assert len(joined) >= 100 and len({n % 32 for _, n in joined if n % 32}) >= 8          # joins inside a word of the store, at many phases
    assert len(MO.sequences_joined_across(text, 65536)) >= 5


GROW_N, GROW_WINDOW = 300000, 65536


def _joined_across(text, window):
    """``motifcases.sequences_joined_across`` for a text whose only '>' begin its headers, with the sequence's index: the cuts of
    ``motifcases.window_cuts`` that fall inside a sequence -> [(index, its bases in front of the cut)].  (Parsed from the sequence's
    own header on, not from the text's first byte: the same answer for a text of 600 000 lines in a second.)"""
    out = []
    for cut in MO.window_cuts(text, window):
        rest = text[cut:].lstrip(b"\r\n")
        if rest[:1] in (b">", b""):
            continue
        out.append((text.count(b">", 0, cut) - 1, len(MO.parse_fasta(text[text.rfind(b">", 0, cut):cut])[-1][1])))
    return out


def _grow_build(workdir):
    """test_the_store_grows_under_many_short_sequences' recipe -- 300 000 sequences of one or two bases under names of at most four
    letters, 16 bytes of store each where the store is first given a quarter more than half the file -- with a sequence of a few
    hundred bases over short lines mixed in every thousand, and one more wherever a window of 64 KiB is about to end: that one the
    cut falls into, so nearly every window joins a sequence, most of them in a store that has already grown."""
    os.makedirs(workdir, exist_ok=True)
    rng = np.random.default_rng(4)
    names = [np.base_repr(k, 36).lower().encode() for k in range(GROW_N)]
    bases = MO.random_bases(rng, 2 * GROW_N)
    t, lo = bytearray(), 0          # lo: where the window that is open began
    for k in range(GROW_N):
        if k % 1000 == 500 or len(t) > lo + GROW_WINDOW - 40:
            t.extend(MO.fasta_text([(names[k], MO.random_bases(rng, int(rng.integers(200, 600)), plain=True))], width=int(rng.integers(5, 20))))
        else:
            t.extend(b">" + names[k] + b"\n" + bases[2 * k:2 * k + (2 if k % 31 == 0 else 1)] + b"\n")
        if len(t) > lo + GROW_WINDOW:
            lo = t.rfind(b"\n", lo, lo + GROW_WINDOW) + 1
    text = bytes(t)
    path = os.path.join(workdir, "short.fa")
    with open(path, "wb") as fh:
        fh.write(text)
    return dict(path=path, joined=np.asarray(_joined_across(text, GROW_WINDOW), np.int64).reshape(-1, 2))


def _grow_sampled():
    return list(range(0, 64)) + list(range(64, GROW_N, 997)) + [GROW_N - 1]


def _grow_run(ctx, inp, outdir):
    from spliser_amd import native
    out = {}
    with native.Genome(ctx, inp["path"], GROW_WINDOW) as g:
        out["n_names"] = np.array([len(g.names)], np.int64)
        out["lengths"] = np.asarray(g.lengths, np.int64)
        out["device_bytes"] = np.array([g.stats()["device_bytes"]], np.int64)
        out["bases_sampled"] = np.concatenate([g.bases(k) for k in _grow_sampled()])
        out["bases_joined"] = np.concatenate([g.bases(int(k)) for k in inp["joined"][:, 0]])
    return out


def _grow_want(inp):
    seqs = MO.parse_fasta(open(inp["path"], "rb").read())
    lengths = np.array([len(c) for _, c in seqs], np.int64)
    return {"n_names": np.array([len(seqs)], np.int64), "lengths": lengths, "device_bytes": np.array([int((16 * ((lengths + 31) // 32)).sum())], np.int64),
            "bases_sampled": np.concatenate([seqs[k][1] for k in _grow_sampled()]), "bases_joined": np.concatenate([seqs[int(k)][1] for k in inp["joined"][:, 0]])}


def _grow_nontrivial(inp, w):
    size, lengths, joined = os.path.getsize(inp["path"]), w["lengths"], inp["joined"]
    assert lengths.shape[0] == GROW_N and 16 * GROW_N > 2 * (size // 2 + 4096) + (2 << 20)          # the store must grow: no rounding of the first allocation holds it
    need = size // 2 + 4096
    first = (max(need + need // 4, 4096) + 255) // 256 * 256          # the first allocation, as GenomeLoad::room makes it
    assert int(w["device_bytes"][0]) > 2 * first
    place = np.concatenate(([0], np.cumsum(16 * ((lengths + 31) // 32))))          # 16 bytes per 32 bases, cumulative
    beyond = [(k, n) for k, n in joined.tolist() if n % 32 and place[k] + 16 * (n // 32) >= first]
    assert len(beyond) >= 5 and len({n % 32 for _, n in beyond}) >= 4, beyond          # joined at a non-zero phase, in a word beyond the first allocation
    assert any(place[k] + 16 * (n // 32) < first for k, n in joined.tolist())                # ... and before the store grew, too
    assert all(lengths[k] >= 200 for k, _ in joined.tolist()) and int((lengths >= 200).sum()) >= 300


# ---- the motif kernel: one fused set, its strand bytes written over twice, the tally, the table the bytes imply ----------------------------
MOTIF_CASES = ("planted", "random")
MOTIF_SHIFT = 700


def _motif_extra(n):
    """The six out-of-range rows of test_junction_motifs_of_a_table for a sequence of n bases."""
    return [(-5, 40), (-1, 30), (n - 10, n + 1), (n, n + 50), (10, 12), (2147483000, 2147483600)]


def _motif_build(workdir):
    os.makedirs(workdir, exist_ok=True)
    made = dict(planted=MO.planted_case(), random=MO.random_case(20261021, 5000))
    path = os.path.join(workdir, "two.fa")
    with open(path, "wb") as fh:
        fh.write(MO.fasta_text([(b"planted", made["planted"][0]), (b"none", b""), (b"random", made["random"][0])], width=61))
    out = dict(fasta=path)
    for name in MOTIF_CASES:
        bases, rs, juncs = made[name]
        right = MO.expected(rs, MO.codes_of(bases))[0]
        out[name] = dict(bases=bases, rs=rs, juncs=np.asarray(juncs, np.int64), wrong=np.where(right == 45, 43, 45).astype(np.uint8))          # every byte goes up wrong
    return out


def _rows4(table):
    return np.asarray([r[:4] for r in J.rows(table)], np.int64).reshape(-1, 4)


def _motif_run(ctx, inp, outdir):
    from spliser_amd import native
    out = {}
    with native.Genome(ctx, inp["fasta"]) as g:
        for name in MOTIF_CASES:
            rs, wrong, juncs = inp[name]["rs"], inp[name]["wrong"], inp[name]["juncs"].tolist()
            with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, xs=wrong)], with_strand=True) as soa:
                with ctx.begin_reads() as dr:
                    dr.add_soa(soa, 0)
                    dr.finish()
                    out[name + "_tally"] = dr.motif_strand(g, name)
                    out[name + "_tally_again"] = dr.motif_strand(g, name)          # (a tally buffer that is not cleared: doubled, or 0xA5)
                    out[name + "_table"] = _rows4(dr.junctions(native.STRAND_FROM_XS, 0, 0, 0))
                    out[name + "_strand_tally"] = dr.strand_tally()
                    out[name + "_record_bytes"] = np.array([dr.layout_bytes()[1]], np.int64)
            with ctx.upload_soa([native.ReadArrays(rs.pos - MOTIF_SHIFT, rs.flag, rs.cig_off, rs.cigar, xs=wrong)], with_strand=True) as soa:
                with ctx.begin_reads() as dr:
                    dr.add_soa(soa, 0, MOTIF_SHIFT)
                    dr.finish()
                    out[name + "_shifted_tally"] = dr.motif_strand(g, g.index(name))
                    out[name + "_shifted_table"] = _rows4(dr.junctions(native.STRAND_FROM_XS, 0, 0, 0))
            rows = juncs + _motif_extra(len(inp[name]["bases"]))
            out[name + "_junction_motifs"] = g.junction_motifs(name, [l for l, _ in rows], [r for _, r in rows])
    return out


def _table_of_bytes(rs, bytes_, shift=0):
    return np.asarray([k + (n,) for k, n in sorted(MO.table_by_strand(rs, bytes_, shift).items())], np.int64).reshape(-1, 4)


def _motif_want(inp):
    out = {}
    for name in MOTIF_CASES:
        rs, seq = inp[name]["rs"], MO.codes_of(inp[name]["bases"])
        bytes_, tally = MO.expected(rs, seq)
        out[name + "_tally"] = out[name + "_tally_again"] = out[name + "_shifted_tally"] = tally
        out[name + "_table"] = _table_of_bytes(rs, bytes_)
        # (the table takes a read by its own POS, which the shift has moved below 1 for the first of them; the motif kernel by POS + shift)
        out[name + "_shifted_table"] = _table_of_bytes(samio.ReadSet(rs.pos - MOTIF_SHIFT, rs.flag, rs.cig_off, rs.cigar), bytes_, MOTIF_SHIFT)
        out[name + "_strand_tally"] = np.asarray(S.tally(rs, bytes_), np.int64)
        out[name + "_record_bytes"] = np.zeros(1, np.int64)          # the set stays fused
        rows = inp[name]["juncs"].tolist() + _motif_extra(len(seq))
        out[name + "_junction_motifs"] = np.array([MO.motif_code(seq, l, r)[0] for l, r in rows], np.int64)
    return out


def _motif_nontrivial(inp, w):
    bytes_ = MO.expected(inp["random"]["rs"], MO.codes_of(inp["random"]["bases"]))[0]
    t = w["random_tally"]
    assert min(int((bytes_ == 43).sum()), int((bytes_ == 45).sum()), int(t[9]), int(t[10])) >= 100, t          # +, -, conflicting, no canonical motif
    for name in MOTIF_CASES:
        right = MO.expected(inp[name]["rs"], MO.codes_of(inp[name]["bases"]))[0]
        assert not (inp[name]["wrong"] == right).any()
        assert {43, 45, 63} == set(w[name + "_table"][:, 2].tolist()) and set(range(7)) == set(w[name + "_junction_motifs"].tolist())
    assert int(w["planted_tally"][11]) > 0 and int(w["planted_strand_tally"][2:8].sum()) > 0          # a junction beyond the sequence's end


# ---- one finished set with name keys and strand bytes: the fragment consumers in turn ----------------------------------------------------
FRAG_BASES = CF.LENGTH + 200          # (the planted pair past LENGTH ends at LENGTH + 20: the per-base yardsticks of the counts look this far)
FRAG_GENES = 9
FRAG_INTRON_LENGTH = CF.LENGTH - 900
FRAG_CALLS = 22                       # the calls of _fragset_run that are followed by a look at the records' bytes


def _fragset_build(workdir):
    rng = np.random.default_rng(20261022)
    rs, keys, _ = CF.paired_content(rng)
    _, xs = X.make_tags(rng, rs)
    features = G.random_features(rng, CF.LENGTH - 700, FRAG_GENES, 30)
    return dict(rs=rs, keys=keys, xs=xs, features=features)


def _fragset_run(ctx, inp, outdir):
    from spliser_amd import exoncounts as xc, genecounts as gc, native
    rs, xs, keys, features = inp["rs"], inp["xs"], inp["keys"], inp["features"]
    out, records_bytes = {}, []
    a, _ = gc.gene_maps(*_arrays(features))
    bin_map, _, (bin_gene, _, _) = xc.exon_maps(*_arrays(features), stranded=False)
    introns = [x[3] for x in I.introns_of(features, ".", FRAG_INTRON_LENGTH)]

    def seen():
        records_bytes.append(dr.layout_bytes()[1])

    def coverage(tag, *args, **kw):
        start, end, depth, t = dr.coverage(CF.LENGTH, *args, **kw)
        out[tag + "_start"], out[tag + "_end"], out[tag + "_depth"] = start, end, depth
        out[tag + "_totals"] = np.array([t[k] for k in (native.COVERAGE_FRAGMENT_TOTALS if kw else native.COVERAGE_TOTALS)], np.int64)
        seen()

    with ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, xs=xs, name_key=keys)], with_strand=True, with_keys=True) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            dr.finish()
            seen()
            coverage("coverage")
            coverage("coverage_fragments", fragments=True)
            coverage("coverage_fragments_fr_plus", 1, "+", fragments=True)
            for stranded in (0, 1, native.STRAND_FROM_XS):
                for k, knobs in enumerate(CF.KNOBS):
                    out["junctions_fragments_s%d_knobs%d" % (stranded, k)] = _rows(J.rows(dr.junctions(stranded, *knobs, fragments=True))); seen()
            for trim in TRIMS:
                out["intron_depth_fragments_trim%d" % trim] = dr.intron_depth(FRAG_INTRON_LENGTH, *_tables(introns), trim_percent=trim, fragments=True); seen()
            out["exon_counts_fragments"] = dr.exon_counts(bin_gene.astype(np.uint32), bin_map, fragments=True); seen()
            out["exon_counts"] = dr.exon_counts(bin_gene.astype(np.uint32), bin_map); seen()
            out["gene_counts_fragments"] = dr.gene_counts(FRAG_GENES, a, fragments=True); seen()
            out["gene_counts"] = dr.gene_counts(FRAG_GENES, a); seen()
            mate, counts = dr.mate_table(0, rs.n); seen()
            out["mate"], out["mate_counts"] = mate, np.array([counts[k] for k in native.MATE_COUNTS], np.int64)
            out["junctions"] = _rows(J.rows(dr.junctions(0))); seen()
            out["junctions_from_xs"] = _rows(J.rows(dr.junctions(native.STRAND_FROM_XS))); seen()
            coverage("coverage_again")
            coverage("coverage_fragments_again", fragments=True)
    out["record_bytes_after_every_call"] = np.asarray(records_bytes, np.int64)
    return out


def _fragset_want(inp):
    from spliser_amd import exoncounts as xc
    oracle = _oracle()
    rs, xs, keys, features = inp["rs"], inp["xs"], inp["keys"], inp["features"]
    mate, counts = M.mate_table_of(rs, keys)
    out = {"mate": np.asarray(mate, np.int64), "mate_counts": np.array([counts[k] for k in ("pairable", "paired", "unpaired_mate_mapped")], np.int64)}
    depth, totals = C.depth_of(rs, CF.LENGTH)
    start, end, value = C.runs_of(depth)
    out["coverage_start"], out["coverage_end"], out["coverage_depth"], out["coverage_totals"] = start, end, value, np.array([start.shape[0]] + totals, np.int64)
    for tag, args in (("coverage_fragments", ()), ("coverage_fragments_fr_plus", (1, "+"))):
        (start, end, value), totals = CF.want_of(rs, mate, CF.LENGTH, 0, *args)
        out[tag + "_start"], out[tag + "_end"], out[tag + "_depth"], out[tag + "_totals"] = start, end, value, np.array(totals, np.int64)
    for k in ("start", "end", "depth", "totals"):
        out["coverage_again_" + k], out["coverage_fragments_again_" + k] = out["coverage_" + k], out["coverage_fragments_" + k]
    for stranded in (0, 1, 3):
        for k, knobs in enumerate(CF.KNOBS):
            out["junctions_fragments_s%d_knobs%d" % (stranded, k)] = _rows(CF.table_rows(CF.junction_tables(rs, mate, stranded, knobs, xs=xs if stranded == 3 else None)[0]))
    introns = [x[3] for x in I.introns_of(features, ".", FRAG_INTRON_LENGTH)]
    per_fragment = CF.fragment_depth(rs, mate, FRAG_INTRON_LENGTH)[0]
    for trim in TRIMS:
        out["intron_depth_fragments_trim%d" % trim] = np.asarray([I.stats_of(per_fragment, pieces, trim) for pieces in introns], np.int64).reshape(-1, 4)
    labels = E.labels_of_features(features, FRAG_BASES)
    bins = E.bins_of([labels])
    _, _, (bin_gene, bin_start, bin_end) = xc.exon_maps(*_arrays(features), stranded=False)
    assert list(zip(bin_start.tolist(), bin_end.tolist(), bin_gene.tolist())) == bins          # (the product's bins are the yardstick's)
    number_of = {k: i for i, k in enumerate(bins)}
    out["exon_counts_fragments"] = np.asarray(EF.counts_of(EF.fragment_results(rs, keys, labels, mate=mate), number_of, len(bins)), np.int64)
    out["exon_counts"] = np.asarray(E.counts_of(E.reads_of(rs, labels), number_of, len(bins)), np.int64)
    bases = G.bases_of_features(features, FRAG_BASES)
    out["gene_counts_fragments"] = np.asarray(M.counts_of(M.fragment_results(rs, keys, bases, mate=mate), FRAG_GENES), np.int64)
    out["gene_counts"] = np.asarray(G.counts_of(G.results_of(rs, bases), FRAG_GENES), np.int64)
    out["junctions"] = _rows(oracle.junction_table(rs.pos, rs.flag, rs.cig_off, rs.cigar, 0, 0, 0, 0))
    out["junctions_from_xs"] = _rows(X.yardstick(rs, xs))
    out["record_bytes_after_every_call"] = np.zeros(FRAG_CALLS, np.int64)          # the set stays fused: no records are ever written
    return out


def _fragset_nontrivial(inp, w):
    rs, keys = inp["rs"], inp["keys"]
    CF.assert_covers(rs, keys)
    assert w["mate_counts"][1] // 2 > 100 and w["coverage_fragments_totals"][5] == w["mate_counts"][1] // 2          # pairs, and every pair's union taken
    assert 0 < w["coverage_fragments_fr_plus_totals"][5] < w["coverage_fragments_totals"][5]
    assert int(w["coverage_fragments_totals"][4]) < int(w["coverage_totals"][4]) and w["coverage_totals"][3] > 0      # fewer covered bases per fragment; reads past the end
    assert not np.array_equal(C.expand(w["coverage_start"], w["coverage_end"], w["coverage_depth"], CF.LENGTH),
                              C.expand(w["coverage_fragments_start"], w["coverage_fragments_end"], w["coverage_fragments_depth"], CF.LENGTH))
    mate = [int(m) for m in w["mate"]]
    for stranded in (0, 1):
        for k, knobs in enumerate(CF.KNOBS):
            frag, read, per_read = CF.junction_tables(rs, mate, stranded, knobs)
            assert sum(1 for p in per_read if p and p[1]) >= 1, (stranded, knobs)          # a junction both mates support, counted once
            assert len(frag) > 20 and sum(r[0] for r in frag.values()) < sum(r[0] for r in read.values())
    assert {43, 45, 63} <= set(w["junctions_fragments_s3_knobs0"][:, 2].tolist())
    n_bins = w["exon_counts"].shape[0] - 4
    for k in ("exon_counts", "exon_counts_fragments"):
        assert min(w[k][n_bins:].tolist()) > 0 and int(np.count_nonzero(w[k][:n_bins])) >= 8, k          # every special counter above zero
    assert int(w["exon_counts_fragments"][:n_bins].sum()) < int(w["exon_counts"][:n_bins].sum())
    assert min(w["gene_counts_fragments"][FRAG_GENES:].tolist()) > 0 and int(w["gene_counts_fragments"].sum()) == rs.n - w["mate_counts"][1] // 2
    for trim in TRIMS:
        t = w["intron_depth_fragments_trim%d" % trim]
        assert t.shape[0] > 3 and int(t[:, 1].sum()) > 0


# ---- text in many windows: SPL_SAM_WINDOW_BYTES = 4096 over the files of the text cases, and a command whose FASTA goes up so too ----------
TEXT_WINDOW = 4096


def _text_windows_build(workdir):
    """_text_build's files, a plain-gzip copy of the text, and a BGZF copy in blocks of 1021 bytes: the one block of ``samz`` is one
    window whatever the variable says, these are four to a window."""
    inp = _text_build(workdir)
    text = open(inp["sam"], "rb").read()
    inp["samgz"], inp["samz_small"] = inp["sam"] + ".plain.gz", inp["sam"] + ".small.gz"
    with open(inp["samgz"], "wb") as fh:
        fh.write(Z.gz(text))
    with open(inp["samz_small"], "wb") as fh:
        fh.write(Z.bgzf(text))
    return inp


def _in_windows(run):
    def inner(ctx, inp, outdir):
        with _env(SPL_SAM_WINDOW_BYTES=TEXT_WINDOW):
            return run(ctx, inp, outdir)
    return inner


def _fragments_bgzf_windows_run(ctx, inp, outdir):
    out = _fragments_run("samz")(ctx, inp, outdir)
    out["genecounts_of_small_blocks.tsv"] = _fragments_run("samz_small")(ctx, inp, outdir)["genecounts.tsv"]
    return out


def _fragments_bgzf_windows_want(inp):
    text = _fragments_want(inp)["genecounts.tsv"]
    return {"genecounts.tsv": text, "genecounts_of_small_blocks.tsv": text}


def _n_text_windows(inp):
    text = open(inp["sam"], "rb").read()
    begin = 0
    while text[begin:begin + 1] == b"@":
        begin = text.index(b"\n", begin) + 1
    plan, stopped = W.window_plan(text, begin, TEXT_WINDOW, W.STOP)
    assert not stopped and max(len(line) for line in text.split(b"\n")) < TEXT_WINDOW // 8
    return len(plan)


def _text_windows_nontrivial(then):
    def inner(inp, w):
        assert _n_text_windows(inp) >= 8
        import gzip
        text = open(inp["sam"], "rb").read()
        assert gzip.decompress(open(inp["samgz"], "rb").read()) == text and gzip.decompress(open(inp["samz_small"], "rb").read()) == text
        assert open(inp["samz_small"], "rb").read().count(b"\x1f\x8b\x08\x04") > 4 * 8          # (BGZF blocks: many windows of them)
        then(inp, w)
    return inner


E2E_NAMES = ["c1", "c2", "c3"]


def _e2e_motif_build(workdir):
    os.makedirs(workdir, exist_ok=True)
    made = [MO.random_case(100 + k, 1200) for k in range(len(E2E_NAMES))]
    sets = [(c, rs) for c, (_, rs, _) in zip(E2E_NAMES, made)]
    bases = {c: b for c, (b, _, _) in zip(E2E_NAMES, made)}
    sam, fasta = os.path.join(workdir, "plain.sam"), os.path.join(workdir, "g.fa")
    samio.write_sam(sam, E2E_NAMES, [len(bases[c]) for c in E2E_NAMES], sets)
    with open(fasta, "wb") as fh:          # (in another order than the header's, with a sequence nobody aligned to)
        fh.write(MO.fasta_text([(b"c3", bases["c3"]), (b"extra", b"ACGTNNNN" * 40), (b"c1", bases["c1"]), (b"c2", bases["c2"])], width=70))
    return dict(sam=sam, fasta=fasta, sets=sets, bases=[bases[c] for c in E2E_NAMES])


def _e2e_motif_run(ctx, inp, outdir):
    from spliser_amd import cli, process as proc
    bed = os.path.join(outdir, "motif.bed")
    with _env(SPL_SAM_WINDOW_BYTES=TEXT_WINDOW):          # (the SAM text's windows and the FASTA's: GenomeLoad's default window is the same variable)
        if cli.main(["junctions", "-B", inp["sam"], "-o", bed, "--genome", inp["fasta"], "--strandFromMotif", "-a", "0", "-m", "0", "-M", "0"]) != 0:
            raise RuntimeError("junctions --strandFromMotif failed")
        proc.wait_deferred_close()
    rows = []
    for line in open(bed).read().splitlines()[1:]:
        c = line.split("\t")
        sizes = c[10].split(",")
        rows.append((E2E_NAMES.index(c[0]), int(c[1]) + int(sizes[0]), int(c[2]) - int(sizes[1]), ord(c[5]), int(c[4])))
    return {"bed_rows": np.asarray(rows, np.int64).reshape(-1, 5)}


def _e2e_motif_want(inp):
    rows = []
    for k, ((_, rs), bases) in enumerate(zip(inp["sets"], inp["bases"])):
        rows += [(k,) + tuple(r) for r in _table_of_bytes(rs, MO.expected(rs, MO.codes_of(bases))[0]).tolist()]
    return {"bed_rows": np.asarray(rows, np.int64).reshape(-1, 5)}


def _e2e_motif_nontrivial(inp, w):
    rows = w["bed_rows"]
    assert set(rows[:, 0].tolist()) == {0, 1, 2} and {43, 45, 63} == set(rows[:, 3].tolist()) and rows.shape[0] > 150 and int(rows[:, 4].max()) > 3
    assert len(MO.window_cuts(open(inp["fasta"], "rb").read(), TEXT_WINDOW)) >= 8 and os.path.getsize(inp["sam"]) > 8 * TEXT_WINDOW
    assert len(MO.sequences_joined_across(open(inp["fasta"], "rb").read(), TEXT_WINDOW)) >= 8


# ---- two lanes: two shards' passes side by side on one context -----------------------------------------------------------------------
LANE_MODES = [(0, 0), (1, 0), (2, 1), (1, 1)]          # (stranded, combine) of the four steps
LANE_EARLY = 2                                          # the step whose first shard is read down before the barrier


def _lanes_build(workdir):
    return dict(cases=[L.tile_case("class_change_%d" % (L.TILE + 1)), L.window_case(L.WIN)])


def _lanes_run(ctx, inp, outdir):
    from spliser_amd import native
    out, dev = {}, []

    def results(step, n):
        ds = dev[n][0]
        for j, a in enumerate(ds.counters()):
            out["step%d_shard%d_counter%d" % (step, n, j)] = np.asarray(a)
        for j, a in enumerate(ds.sse_results()):
            out["step%d_shard%d_sse%d" % (step, n, j)] = np.asarray(a)

    with _env(SPL_FORCE_CHUNK=L.CHUNK):
        try:
            for case in inp["cases"]:
                soa = ctx.upload_soa([native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar) for rs, _ in case.segments])
                dev.append([None, None, soa])
                dev[-1][0] = ctx.upload_sites(case.table.sites())
                dev[-1][1] = ctx.layout_read_segments(soa, [shift for _, shift in case.segments])
            for step, (stranded, combine) in enumerate(LANE_MODES):
                for ds, dr, _ in dev:
                    dr.relayout()
                    ctx.count_launch(ds, dr, stranded, combine, 0)
                    ctx.sse_launch(ds, (stranded + combine) % 2 == 0)
                if step == LANE_EARLY:          # the second shard's pass still queued behind it
                    results(step, 0)
                ctx.pass_barrier()
                for n in range(len(dev)):
                    if not (step == LANE_EARLY and n == 0):
                        results(step, n)
            out["record_bytes"] = np.array([dr.layout_bytes()[1] for _, dr, _ in dev], np.int64)
        finally:
            ctx.sync()
            for ds, dr, soa in dev:
                for h in (dr, ds, soa):
                    if h is not None:
                        h.free()
    return out


def _lanes_want(inp):
    oracle, out = _oracle(), {}
    for n, case in enumerate(inp["cases"]):
        t, r = case.table, case.reads
        for step, (stranded, combine) in enumerate(LANE_MODES):
            counts = oracle.check_bam(t.pos, t.strand, t.part_off, t.part_pos, t.comp_off, t.comp_pos, r.pos, r.flag, r.cig_off, r.cigar, stranded, combine)
            sse = oracle.beta2_sse(t.pos, t.part_off, t.part_pos, t.part_site, t.alpha, t.edge_cnt, counts[0], counts[1], counts[2], (stranded + combine) % 2 == 0)
            for j, a in enumerate(counts):
                out["step%d_shard%d_counter%d" % (step, n, j)] = np.asarray(a)
            for j, a in enumerate(sse):
                out["step%d_shard%d_sse%d" % (step, n, j)] = np.asarray(a)
    out["record_bytes"] = np.zeros(len(inp["cases"]), np.int64)          # both sets are fused
    return out


def _lanes_nontrivial(inp, w):
    tile, window = inp["cases"]
    assert tile.reads.n > L.CHUNK and tile.reads.n > L.TILE and window.table.n > L.WIN          # more than one chunk and one tile; more than one window
    assert len(set(LANE_MODES)) == len(LANE_MODES) and all(a != b for a, b in zip(LANE_MODES, LANE_MODES[1:]))
    for step in range(len(LANE_MODES)):
        for n in (0, 1):
            assert int(w["step%d_shard%d_counter0" % (step, n)].sum()) > 0 and int(w["step%d_shard%d_counter1" % (step, n)].sum()) > 0, (step, n)
    assert any(not np.array_equal(w["step0_shard%d_counter%d" % (n, j)], w["step1_shard%d_counter%d" % (n, j)]) for n in (0, 1) for j in (0, 1, 2))          # the mode matters


# ---- the list -----------------------------------------------------------------------------------------------------------------
def cases():
    out = [_count_case(k, name, make) for k, (name, make) in enumerate(COUNT_CASES)]
    out.append(PCase("decode_shuffled_all_switches", _decode_build, _decode_shuffled_run, lambda inp: _decode_want(inp, inp["mixed"], True, True), _decode_nontrivial))
    out.append(PCase("decode_sorted_in_three_shares", _decode_build, _decode_shares_run, _decode_shares_want, _decode_nontrivial))
    out.append(PCase("text_fragments_sam", _text_build, _fragments_run("sam"), _fragments_want, _fragments_nontrivial))
    out.append(PCase("text_fragments_bgzf_sam", _text_build, _fragments_run("samz"), _fragments_want, _fragments_nontrivial))
    out.append(PCase("text_coverage_sam", _text_build, _text_coverage_run, _text_coverage_want, _text_coverage_nontrivial))
    out.append(PCase("one_set_every_consumer", _oneset_build, _oneset_run, _oneset_want, _oneset_nontrivial))
    out += [_junction_case(name) for name in ("record_classes", "wave_merge", "hash")]
    out.append(PCase("end_to_end_process_kat2", lambda workdir: {}, _kat2_run, _kat2_want, _kat2_nontrivial))
    out.append(PCase("end_to_end_combine_a", lambda workdir: {}, _combine_run, _combine_want, _combine_nontrivial))
    # what came after the list was first written: the genome, the motif kernel, the fragment variants, text in many windows, two lanes
    out.append(PCase("genome_pack_windows", _genome_pack_build, _genome_pack_run, _genome_pack_want, _genome_pack_nontrivial))
    out.append(PCase("genome_store_growth", _grow_build, _grow_run, _grow_want, _grow_nontrivial))
    out.append(PCase("motif_one_set", _motif_build, _motif_run, _motif_want, _motif_nontrivial))
    out.append(PCase("one_set_fragment_consumers", _fragset_build, _fragset_run, _fragset_want, _fragset_nontrivial))
    out.append(PCase("text_windows_fragments_sam", _text_windows_build, _in_windows(_fragments_run("sam")), _fragments_want, _text_windows_nontrivial(_fragments_nontrivial)))
    out.append(PCase("text_windows_fragments_bgzf_sam", _text_windows_build, _in_windows(_fragments_bgzf_windows_run), _fragments_bgzf_windows_want,
                     _text_windows_nontrivial(_fragments_nontrivial)))
    out.append(PCase("text_windows_fragments_gzip_sam", _text_windows_build, _in_windows(_fragments_run("samgz")), _fragments_want, _text_windows_nontrivial(_fragments_nontrivial)))
    out.append(PCase("text_windows_coverage_sam", _text_windows_build, _in_windows(_text_coverage_run), _text_coverage_want, _text_windows_nontrivial(_text_coverage_nontrivial)))
    out.append(PCase("end_to_end_junctions_from_motif", _e2e_motif_build, _e2e_motif_run, _e2e_motif_want, _e2e_motif_nontrivial))
    out.append(PCase("lanes_two_shards", _lanes_build, _lanes_run, _lanes_want, _lanes_nontrivial))
    return out


CASES = cases()
NAMES = [c.name for c in CASES]
_WORK, _INPUTS, _WANTS = [], {}, {}


def case(name):
    return CASES[NAMES.index(name)]


def workdir():
    if not _WORK:
        _WORK.append(tempfile.mkdtemp(prefix="poisoncases"))
        atexit.register(shutil.rmtree, _WORK[0], True)
    return _WORK[0]


def inputs_of(name):
    """The case's inputs, built once a process (its files under a directory that goes with the process)."""
    if name not in _INPUTS:
        _INPUTS[name] = case(name).build(os.path.join(workdir(), name))
    return _INPUTS[name]


def want_of(name):
    """The yardstick's results, computed once a process and left unchanged."""
    if name not in _WANTS:
        _WANTS[name] = normalised(case(name).want(inputs_of(name)))
    return _WANTS[name]


# ---- results: how they are kept, and how they are compared ----------------------------------------------------------------------
def normalised(results):
    """{key: array or bytes} -> {key: ndarray}: texts as their bytes, integers as int64 (uint64 as it is), floats as float64."""
    out = {}
    for k, v in results.items():
        if isinstance(v, (bytes, bytearray, str)):
            v = np.frombuffer(v.encode() if isinstance(v, str) else bytes(v), np.uint8)
        v = np.asarray(v)
        if v.dtype.kind == "b" or (v.dtype.kind in "iu" and v.dtype != np.uint64):
            v = v.astype(np.int64)
        elif v.dtype.kind == "f":
            v = v.astype(np.float64)
        out[k] = v
    return out


def mismatches(got, want):
    """What of ``got`` is not ``want`` (both normalised), as a list of texts; empty when everything is equal.  Every array is held
    bit for bit (NaN equal to NaN), the counting pass's SSE besides to the 1e-9 BASELINE.json states, as
    test_gpu_kernel_limits._assert_sse holds it."""
    bad = []
    for k in sorted(set(got) | set(want)):
        if k not in got or k not in want:
            bad.append("%s: %s" % (k, "missing" if k not in got else "not expected"))
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.dtype.kind in "iu" and w.dtype.kind in "iu" and g.dtype != w.dtype:
            g, w = g.astype(np.uint64), w.astype(np.uint64)          # (name keys and mate words against Python's integers)
        if g.dtype.kind != w.dtype.kind:
            bad.append("%s: %s where %s was expected" % (k, g.dtype, w.dtype))
        elif g.shape != w.shape:
            bad.append("%s: shape %s where %s was expected" % (k, g.shape, w.shape))
        elif not np.array_equal(g, w, equal_nan=w.dtype.kind == "f"):
            same = (g == w) | ((g != g) & (w != w)) if w.dtype.kind == "f" else g == w
            where = np.flatnonzero(~same.ravel())
            bad.append("%s: %d of %d entries differ, the first at %d: %r where %r was expected"
                       % (k, where.size, g.size, int(where[0]), g.ravel()[where[0]].item(), w.ravel()[where[0]].item()))
        elif k.endswith("_sse3") and not np.all(np.abs(g - w)[np.isfinite(w)] <= 1e-9):
            bad.append("%s: beyond 1e-9" % k)
    return bad


def load(path):
    with np.load(path) as z:
        return normalised({k: z[k] for k in z.files})


def fingerprint(x, h=None):
    """A digest of a case's inputs: arrays by their bytes, files by their content (not their path), objects by their attributes."""
    top = h is None
    h = hashlib.sha256() if top else h
    if isinstance(x, np.ndarray):
        h.update(str((x.dtype.str, x.shape)).encode() + np.ascontiguousarray(x).tobytes())
    elif isinstance(x, dict):
        for k in sorted(x, key=str):
            h.update(str(k).encode())
            fingerprint(x[k], h)
    elif isinstance(x, (list, tuple)):
        h.update(b"[%d" % len(x))
        for v in x:
            fingerprint(v, h)
    elif isinstance(x, str) and os.path.isfile(x):
        with open(x, "rb") as fh:
            h.update(fh.read())
    elif isinstance(x, (str, bytes, int, float, bool, type(None), np.generic)):
        h.update(repr(x).encode())
    elif hasattr(x, "__dict__") or hasattr(x, "__slots__"):
        names = list(vars(x)) if hasattr(x, "__dict__") else [k for k in x.__slots__ if hasattr(x, k)]
        fingerprint({k: getattr(x, k) for k in names if not callable(getattr(x, k))}, h)
    else:
        raise TypeError("no fingerprint for %r" % type(x))
    return h.hexdigest() if top else None


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def _run_pass(ctx, names, outdir, progress, seconds):
    os.makedirs(outdir, exist_ok=True)
    for name in names:
        progress.write("begin %s\n" % name)
        progress.flush()
        t0 = time.time()
        scratch = tempfile.mkdtemp(prefix=name + ".", dir=workdir())
        got = normalised(case(name).run(ctx, inputs_of(name), scratch))
        np.savez(os.path.join(outdir, name + ".npz"), **got)
        seconds[os.path.relpath(os.path.join(outdir, name))] = round(time.time() - t0, 3)
        progress.write("end %s\n" % name)
        progress.flush()


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--twice", action="store_true")
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--list", action="store_true")
    args = ap.parse_args(argv)
    if args.list:
        print("\n".join(NAMES))
        return 0
    if not args.out:
        ap.error("--out DIR")
    names = [n for n in NAMES if not args.only or n in args.only]
    os.makedirs(args.out, exist_ok=True)
    from spliser_amd import native
    pool, seconds = {}, {}
    t0 = time.time()
    for name in names:          # (inputs first: what follows is the device's time)
        inputs_of(name)
    pool["build_s"] = round(time.time() - t0, 3)
    with open(os.path.join(args.out, "progress.log"), "w") as progress:
        with native.Context(0) as ctx:
            _run_pass(ctx, names, args.out, progress, seconds)
            pool["after_first_pass"] = native.devmem_stats()
            if args.twice:
                _run_pass(ctx, names[::-1], os.path.join(args.out, "second"), progress, seconds)
                pool["after_second_pass"] = native.devmem_stats()
            progress.write("begin probes\n")
            progress.flush()
            first, cap1 = native.devmem_probe(ctx, PROBE_BYTES)
            pool["after_first_probe"] = native.devmem_stats()
            second, cap2 = native.devmem_probe(ctx, PROBE_BYTES)
            pool["after_second_probe"] = native.devmem_stats()
            pool["probe_capacities"] = [cap1, cap2]
            pool["capacities_by_request"] = [[b, native.devmem_probe(ctx, b, room=0)[1]] for b in PROBE_SIZES]
            np.savez_compressed(os.path.join(args.out, "probes.npz"), first=first, second=second)
            progress.write("end probes\n")
            progress.flush()
    pool["seconds"], pool["wall_s"] = seconds, round(time.time() - t0, 3)
    with open(os.path.join(args.out, "pool.json"), "w") as fh:
        json.dump(pool, fh, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
