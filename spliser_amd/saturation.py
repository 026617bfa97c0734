"""``saturation`` -- how many junctions and how many of SpliSER's sites a library shows at nested subsamples of its reads, from ONE
decode, on the GPU.

Not part of SpliSER v0.1.8.  Its README explains ``minReads`` (``combineShallow -r``, ``output -r``, diffSpliSER's filter: a site
whose alpha + beta1 + beta2Simple is below 10 is dropped) and leaves the user to find out how many sites of a library pass, and
whether more would with more reads.  The usual instrument, RSeQC's ``junction_saturation.py``, is a Python loop over a sorted file
that counts junctions, not sites; the SpliSER-specific one is ``samtools view -s`` twenty times with ``regtools`` and ``process``
behind each.  Here the reads are decoded once, with their name keys; step ``k`` of ``K`` is the read set the subsampling rule keeps
at threshold ``(k << 32) // K`` (``spl_reads_subsample``: a read's decision is a hash of its name and the seed, so mates stay
together, the kept sets are nested and the same names are kept whatever the file's order or container), and row ``k`` is what
``junctions``, ``process`` without ``-b`` and the decode would report on a file that holds exactly those reads.

Parity with RSeQC / samtools -s is not claimed: their choices of reads are others, and mean as little for a random subset.

Steps run descending: step k's set of a chromosome is selected from step k + 1's (nested sets: the same reads, less work), which
is then freed -- at most two sets of a chromosome are alive at once.  Per step the path is the one ``process`` without ``-b``
takes, without its files: every chromosome's junction table from its set, the site table from those arrays
(``process._site_table``), then per chromosome the counting pass at shift 0.  No verdict is given: what counts as "saturated" is the
user's call.
"""
import contextlib
import time

import numpy as np

from . import native, process as _process, readsets

HEADER = "step\tfraction\treads\tjunctions\tjunctions_minReads\tjunction_reads\tsites\tsites_minReads\n"
SUFFIX = ".saturation.tsv"
ALL = native.SUBSAMPLE_ALL


def thresholds(steps):
    """T_k = (k << 32) // K for k = 1 .. K: the last one keeps every read."""
    return [(k << 32) // steps for k in range(1, steps + 1)]


def check(steps, minReads, strandedType):
    if not 1 <= int(steps) <= 100:
        raise ValueError("saturation: --steps must be in 1..100")
    if int(minReads) < 1:
        raise ValueError("saturation: -r / --minReads must be at least 1")
    if strandedType == "auto":
        raise ValueError("saturation: -s auto is not taken here: the `strandedness` command tells whether the library is fr or rf")


def _row_of_step(ctx, sets, chroms, stranded, isStranded, strandedType, knobs, qChrom, minReads, spent, dedup=False):
    """One row's six numbers from the step's sets ({chrom: DeviceReads}): the path of ``process`` without ``-b``, without its files.
    ``dedup``: from the sets without their duplicate fragments, made here and freed here; a seventh number, the reads before."""
    if dedup:
        t0 = time.perf_counter()
        before, left = sum(s.n for s in sets.values()), {}
        try:
            for chrom, dr in sets.items():
                left[chrom] = dr.dedup()[0]
            spent["selections_s"] += time.perf_counter() - t0
            return _row_of_step(ctx, {c: s for c, s in left.items() if s.n}, chroms, stranded, isStranded, strandedType, knobs, qChrom, minReads, spent) + (before,)
        finally:
            for s in left.values():
                s.free()
    t0 = time.perf_counter()
    tables = {c: sets[c].junctions(stranded, *knobs) for c in chroms if c in sets}
    t1 = time.perf_counter()
    n_junctions = sum(len(t["left"]) for t in tables.values())
    n_junctions_min = sum(int((t["count"] >= minReads).sum()) for t in tables.values())
    junction_reads = sum(int(t["count"].astype(np.int64).sum()) for t in tables.values())
    rows = [(c, tables[c]) for c in chroms if c in tables and len(tables[c]["left"])]
    table = _process._site_table(None, "All", qChrom, 0, None, "gene", isStranded, strandedType, lambda m: None, rows_of_bam=lambda: rows)
    t2 = time.perf_counter()
    n_sites = n_sites_min = 0
    for chrom in table.chrom_index:
        if not (qChrom == chrom or qChrom == "All"):
            continue
        arr = table.chrom_arrays(chrom)
        if arr.n == 0:
            continue
        n_sites += arr.n
        with ctx.upload_sites(native.SiteArrays.from_chrom(arr)) as ds:
            with _set_or_none(ctx, sets.get(chrom)) as dr:
                ctx.count_launch(ds, dr, stranded, 0)
                ctx.sse_launch(ds, False)
                beta1, _, _ = ds.counters()
                beta2_simple = ds.sse_results()[0]
        total = np.asarray(arr.alpha, np.int64) + np.asarray(beta1, np.int64)[:arr.n] + np.asarray(beta2_simple, np.int64)[:arr.n]
        n_sites_min += int((total >= minReads).sum())
    t3 = time.perf_counter()
    spent["junction_tables_s"] += t1 - t0
    spent["site_tables_s"] += t2 - t1
    spent["counting_s"] += t3 - t2
    return sum(s.n for s in sets.values()), n_junctions, n_junctions_min, junction_reads, n_sites, n_sites_min


@contextlib.contextmanager
def _set_or_none(ctx, dr):
    """``dr``, or a finished set without a read for a chromosome that has sites and no set (it cannot: its junctions came from reads)."""
    if dr is not None:
        yield dr
        return
    with ctx.begin_reads() as empty:
        yield empty.finish()


def saturation(inBAM, outputPath, steps=20, seed=0, minReads=10, qChrom="All", isStranded=False, strandedType=None, minAnchor=8, minIntron=70, maxIntron=500000,
               anyOrder=False, gpuDecode=None, devices=(0,), threads=0, log=None, minMapQ=0, requireFlags=0, excludeFlags=0, timings=None, dedup=False):
    """Writes ``<outputPath>.saturation.tsv`` -- a row per step k = 1 .. ``steps``: the fraction k / steps, the placed reads kept, the
    junctions (BED lines), those whose score is at least ``minReads``, the sum of the scores, the sites (rows of ``.SpliSER.tsv``) and
    those with alpha_count + beta1_count + beta2Simple_count >= ``minReads`` -- and returns the rows.  ``timings`` (a dict, or None):
    gets the seconds of the decode, the selections, the junction tables, the site tables (host) and the counting passes.  ``dedup``:
    every step's selected set is deduplicated (``DeviceReads.dedup``) before its row is made -- the kept sets are not nested under
    dedup, so the chain of selections stays as it is and the deduplicated sets live for their step only --, the table gets one more
    column, ``reads_before_dedup``, and a returned row a seventh number."""
    log = _process.logger(log)
    check(steps, minReads, strandedType)
    steps, seed, minReads = int(steps), int(seed), int(minReads)
    if not 0 <= seed < 1 << 64:
        raise ValueError("saturation: --seed must be in 0 .. 2^64 - 1")
    stranded = _process.stranded_code("saturation", isStranded, strandedType)
    knobs = (int(minAnchor), int(minIntron), int(maxIntron))
    if min(knobs) < 0:
        raise ValueError("minAnchor / minIntron / maxIntron must not be negative")
    devices = _process.one_device(devices, log, "saturation")
    options = _process.DecodeOptions(_process.read_filter(minMapQ, requireFlags, excludeFlags), any_order=bool(anyOrder), mate_keys=True)
    spent = dict(decode_s=0.0, selections_s=0.0, junction_tables_s=0.0, site_tables_s=0.0, counting_s=0.0)
    t_begin = time.perf_counter()
    rows = {}
    with _process.decoding(inBAM, devices, gpuDecode, threads, options, log=log) as source:
        _process.wait_decoded(source, anyOrder, log)
        if isinstance(source, native.BamFile) and not source.wait_all():
            raise native.SpliserNativeError(-5, "%s is not sorted by reference: sort it (samtools sort) first, or pass --anyOrder" % inBAM)
        chroms = _process.chroms_of(source, qChrom)
        plans = readsets.plans_of(source, devices, chroms)
        spent["decode_s"] = time.perf_counter() - t_begin
        _process.log_filter(source, options.read_filter, log)
        with native.Context(devices[0]) as ctx, contextlib.ExitStack() as whole:
            # every chromosome's whole set (a decode on the device: its arrays where they lie; reads on the host: up with their keys),
            # each held by a stack of its own: it goes as soon as the first selection from it is made
            held, current = {}, {}
            for _, entries in plans:
                for chrom, add in entries:
                    held[chrom] = whole.enter_context(contextlib.ExitStack())
                    dr = held[chrom].enter_context(readsets.fused_set(ctx, source, chrom, add, with_keys=True))
                    if dr is not None:
                        current[chrom] = dr
                    else:
                        held.pop(chrom).close()
            try:
                for k, threshold in reversed(list(enumerate(thresholds(steps), 1))):
                    t0 = time.perf_counter()
                    for chrom in list(current):
                        if threshold >= ALL:          # (the last step keeps every read: the whole set itself)
                            continue
                        before = current.pop(chrom)
                        try:
                            sel, _ = before.subsample(seed, threshold)
                        finally:          # (the larger set goes: at most two sets of a chromosome are alive, here)
                            if chrom in held:
                                held.pop(chrom).close()
                            else:
                                before.free()
                        if sel.n:
                            current[chrom] = sel
                        else:
                            sel.free()
                    spent["selections_s"] += time.perf_counter() - t0
                    rows[k] = _row_of_step(ctx, current, chroms, stranded, isStranded, strandedType, knobs, qChrom, minReads, spent, dedup=bool(dedup))
                    log("step %d of %d (fraction %r): %d reads, %d junctions (%d with at least %d reads), %d sites (%d with at least %d reads)"
                        % (k, steps, k / steps, rows[k][0], rows[k][1], rows[k][2], minReads, rows[k][4], rows[k][5], minReads))
                    if dedup:
                        log("  (dedup: %d of %d reads removed as duplicates)" % (rows[k][6] - rows[k][0], rows[k][6]))
            finally:
                for chrom, dr in current.items():
                    if chrom not in held:          # (a whole set goes with its stack)
                        dr.free()
    with open(outputPath + SUFFIX, "w") as out:
        out.write(HEADER[:-1] + "\treads_before_dedup\n" if dedup else HEADER)
        for k in range(1, steps + 1):
            out.write("%d\t%r\t%s\n" % (k, k / steps, "\t".join("%d" % v for v in rows[k])))
    if steps % 2 == 0:
        n_full, n_half = rows[steps][5], rows[steps // 2][5]
        log("sites with at least %d reads: %d at full depth, %d (%s %%) at half the depth"
            % (minReads, n_full, n_half, "%.1f" % (100.0 * n_half / n_full) if n_full else "-"))
    spent["total_s"] = time.perf_counter() - t_begin
    if timings is not None:
        timings.update(spent)
    return [rows[k] for k in range(1, steps + 1)]
