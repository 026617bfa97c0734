"""The device side of the subsampling tests: a case of ``subsamplecases.py`` goes up with its keys (``upload_soa(with_keys=True)``), is
selected on the device (``DeviceReads.subsample``), and everything that reads a finished fused set reads the selected one -- the
junction table, the coverage runs, the mate tables and a counting pass's counters -- so that every carried array is held: the
same calls on a set uploaded from the numpy-masked host arrays have to give the same numbers.

Run as a program it is the driver of ``test_gpu_subsample.py``'s child process: every case once, what the SELECTED sets gave saved
as ``<out>/<case>.npz`` (the parent holds them against what it computed itself, exactly)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import subsamplecases as S          # noqa: E402
from spliser_amd import fast_sites, native, sites          # noqa: E402

SHIFT = 7          # segment k of a set is moved by SHIFT * k


def _arrays(rs, with_strand):
    return native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, xs=rs.xs if with_strand else None, name_key=rs.keys)


class fused(object):
    """``segs`` ([Reads]) as one finished fused set with keys (and strand bytes), for the length of a ``with``."""

    def __init__(self, ctx, segs, with_strand):
        self.ctx, self.segs, self.with_strand = ctx, segs, with_strand

    def __enter__(self):
        self.soa = self.ctx.upload_soa([_arrays(rs, self.with_strand) for rs in self.segs], with_keys=True, with_strand=self.with_strand)
        self.dr = self.ctx.begin_reads()
        try:
            for k in range(len(self.segs)):
                self.dr.add_soa(self.soa, k, SHIFT * k)
            return self.dr.finish()
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        self.dr.free()
        self.soa.free()


def length_of(segs):
    return 1 + max([0] + [int(rs.pos.max()) + 12000 + SHIFT * len(segs) for rs in segs if rs.n])


def site_arrays(ctx, segs):
    """A small site table for the case: from the junctions of ALL its reads -> ``native.SiteArrays`` or None (no junction)."""
    with fused(ctx, segs, False) as dr:
        t = dr.junctions(0, 0, 0, 0) if dr.n else None
    if t is None or not len(t["left"]):
        return None
    table = fast_sites.build_from_arrays(sites.GeneBins(), False, [("c", t["left"], t["right"], t["strand"], t["count"])])
    if table is None:
        return None
    table.find_competitors()
    return native.SiteArrays.from_chrom(table.chrom_arrays("c"))


def views(ctx, dr, seg_reads, with_strand, length, site):
    """What the consumers of a finished fused set say of ``dr``, whose segments with reads have ``seg_reads`` reads -> {name: array}."""
    out = {}
    for mode in ((native.STRAND_FROM_XS, 1) if with_strand and dr.n else (1, 0)):          # (a set without a read has no strand bytes)
        for k, v in dr.junctions(mode, 0, 0, 0).items():
            out["junctions%d_%s" % (mode, k)] = v
    start, end, depth, totals = dr.coverage(length)
    out.update(cov_start=start, cov_end=end, cov_depth=depth, cov_totals=np.array([totals[k] for k in native.COVERAGE_TOTALS], np.int64))
    for seg, n in enumerate([n for n in seg_reads if n]):
        mate, counts = dr.mate_table(seg, n)
        out["mate%d" % seg] = mate
        out["mate%d_counts" % seg] = np.array([counts[k] for k in native.MATE_COUNTS], np.int64)
    if site is not None:
        with ctx.upload_sites(site) as ds:
            ctx.count_launch(ds, dr, 0, 0)
            ctx.sse_launch(ds, False)
            for k, v in enumerate(ds.counters()):
                out["counters%d" % k] = v
            for k, v in enumerate(ds.sse_results()):
                out["sse%d" % k] = v
    return out


def want_of(ctx, segs, seed, threshold, with_strand, site=None, length=None):
    """By the restatement and numpy: the kept reads per segment, the index, and the views of the masked arrays' set."""
    masks = [rs.mask(seed, threshold) for rs in segs]
    base = np.concatenate(([0], np.cumsum([rs.n for rs in segs]))).astype(np.int64)
    kept = [rs.masked(m) for rs, m in zip(segs, masks)]
    out = dict(kept_per_seg=np.array([int(m.sum()) for rs, m in zip(segs, masks) if rs.n], np.int64),
               index=np.concatenate([base[k] + np.flatnonzero(m) for k, m in enumerate(masks)] + [np.zeros(0, np.int64)]).astype(np.uint32))
    with fused(ctx, kept, with_strand) as dr:
        out.update(views(ctx, dr, [rs.n for rs in kept], with_strand, length_of(segs) if length is None else length, site))
    return out


def got_of(ctx, segs, seed, threshold, with_strand, site=None, length=None):
    """By the device: ``subsample`` of the whole set, the source freed FIRST, then the views of the selected set."""
    src = fused(ctx, segs, with_strand)
    dr = src.__enter__()
    try:
        sel, kept, index = dr.subsample(seed, threshold, with_index=True)
    finally:
        src.__exit__()
    try:
        out = dict(kept_per_seg=kept, index=index)
        assert sel.n == int(kept.sum()) and (not sel.n or (sel.has_mate_keys() and sel.has_strand() == bool(with_strand)))
        seg_reads = [int(v) for v in kept]
        out.update(views(ctx, sel, seg_reads, with_strand, length_of(segs) if length is None else length, site))
    finally:
        sel.free()
    return out


def mismatches(got, want):
    bad = []
    for k in sorted(set(got) | set(want)):
        if k not in got or k not in want:
            bad.append("%s: only in %s" % (k, "what was wanted" if k in want else "what the device gave"))
        elif got[k].shape != want[k].shape or got[k].dtype != want[k].dtype or got[k].tobytes() != want[k].tobytes():
            bad.append("%s: %s %s, wanted %s %s" % (k, got[k].dtype, got[k][:8], want[k].dtype, want[k][:8]))
    return bad


def case_list(tile):
    """-> [(name, segs, seed, threshold, with_strand)]: every case with and without strand bytes."""
    return [("%s_%s" % (name, "xs" if ws else "plain"), segs, seed, threshold, ws) for name, segs, seed, threshold in S.all_cases(tile) for ws in (True, False)]


def main(argv):
    out = argv[argv.index("--out") + 1]
    os.makedirs(out, exist_ok=True)
    with native.Context(0) as ctx:
        for name, segs, seed, threshold, with_strand in case_list(native.subsample_tile()):
            with open(os.path.join(out, "progress.log"), "a") as fh:
                fh.write(name + "\n")
            got = got_of(ctx, segs, seed, threshold, with_strand, site_arrays(ctx, segs))
            np.savez(os.path.join(out, name + ".npz"), **got)
    with open(os.path.join(out, "pool.json"), "w") as fh:
        json.dump(native.devmem_stats(), fh)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
