"""The device side of the duplicate tests: a case of ``dupcases.py`` goes up with its keys, its marks are made on the device twice
over (``DeviceReads.duplicates``), the set is deduplicated (``DeviceReads.dedup``, and once more: nothing goes), and everything
that reads a finished fused set reads the deduplicated one -- ``subsample_device.views`` and the gene counts, per read and per
fragment.  ``want_of`` says the same by the restatement and numpy: the marks, and the same calls on a set uploaded from the
masked host arrays.

Run as a program it is the driver of ``test_gpu_duplicates.py``'s child process: every case once, what the device gave saved as
``<out>/<case>.npz`` (the parent holds them against what it computed itself, exactly)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import dupcases as D          # noqa: E402
import subsample_device as V          # noqa: E402
from spliser_amd import native          # noqa: E402

N_GENES = 3
GENE_MAP = (np.arange(0, 12000, 250, dtype=np.int32), np.array([(0, 1, 2, 0xFFFFFFFF, 3, 0)[k % 6] for k in range(48)], np.uint32))


def _consumers(ctx, dr, seg_reads, with_strand, length):
    out = V.views(ctx, dr, seg_reads, with_strand, length, None)
    out["genes"] = dr.gene_counts(N_GENES, GENE_MAP)
    out["genes_fragments"] = dr.gene_counts(N_GENES, GENE_MAP, fragments=True)
    return out


def want_of(ctx, segs, with_strand):
    """By the restatement and numpy."""
    out, masks = {}, []
    for k, rs in enumerate([rs for rs in segs if rs.n]):
        dup, counts, hist = D.duplicates(rs, rs.keys.tolist())
        out.update({"dup%d" % k: dup, "counts%d" % k: np.array([counts[c] for c in D.COUNTS], np.int64), "hist%d" % k: hist})
    for rs in segs:
        masks.append(~D.duplicates(rs, rs.keys.tolist())[0])
    base = np.concatenate(([0], np.cumsum([rs.n for rs in segs]))).astype(np.int64)
    kept = [rs.masked(m) for rs, m in zip(segs, masks)]
    out.update(kept_per_seg=np.array([int(m.sum()) for rs, m in zip(segs, masks) if rs.n], np.int64),
               index=np.concatenate([base[k] + np.flatnonzero(m) for k, m in enumerate(masks)] + [np.zeros(0, np.int64)]).astype(np.uint32))
    with V.fused(ctx, kept, with_strand) as dr:
        out.update(_consumers(ctx, dr, [rs.n for rs in kept], with_strand, V.length_of(segs)))
    return out


def got_of(ctx, segs, with_strand):
    """By the device: the marks twice, ``dedup`` of the whole set, the source freed FIRST, then the consumers of the deduplicated
    set, and its own ``dedup``."""
    src = V.fused(ctx, segs, with_strand)
    dr = src.__enter__()
    out = {}
    try:
        for k, n in enumerate([rs.n for rs in segs if rs.n]):
            dup, counts, hist = dr.duplicates(k, n)
            again = dr.duplicates(k, n)
            assert np.array_equal(dup, again[0]) and counts == again[1] and np.array_equal(hist, again[2])
            out.update({"dup%d" % k: dup, "counts%d" % k: np.array([counts[c] for c in native.DUP_COUNTS], np.int64), "hist%d" % k: hist})
        sel, kept, index = dr.dedup(with_index=True)
    finally:
        src.__exit__()
    try:
        out.update(kept_per_seg=kept, index=index)
        assert sel.n == int(kept.sum()) and (not sel.n or (sel.has_mate_keys() and sel.has_strand() == bool(with_strand)))
        out.update(_consumers(ctx, sel, [int(v) for v in kept], with_strand, V.length_of(segs)))
        once_more, kept2 = sel.dedup()
        try:
            assert kept2.tolist() == [int(v) for v in kept if v], "a deduplicated set lost reads to dedup"
        finally:
            once_more.free()
    finally:
        sel.free()
    return out


def case_list(tile):
    """-> [(name, segs, with_strand)]: strand bytes on every other case."""
    return [(name, segs, k % 2 == 0) for k, (name, segs) in enumerate(D.all_cases(tile))]


def main(argv):
    out = argv[argv.index("--out") + 1]
    os.makedirs(out, exist_ok=True)
    with native.Context(0) as ctx:
        for name, segs, with_strand in case_list(native.subsample_tile()):
            with open(os.path.join(out, "progress.log"), "a") as fh:
                fh.write(name + "\n")
            np.savez(os.path.join(out, name + ".npz"), **got_of(ctx, segs, with_strand))
    with open(os.path.join(out, "pool.json"), "w") as fh:
        json.dump(native.devmem_stats(), fh)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
