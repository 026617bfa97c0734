"""The plan by which every command visits the reads of an alignment source whose decode has been started
(``process.open_and_decode``): per chromosome one finished read set on a device, taken where the decode left the reads.

  * a file decoded on the device is visited per chromosome where it lies, on the first device (``add_bam``: the sets are fused and
    stay so, nothing is laid out or decoded again);
  * after a decode in shares every device visits ITS piece of a chromosome (``add_bam_share``) -- what the visits add must add over
    reads, and the host adds it up;
  * reads on the host -- a file the host's threads decode, the Python reader's SAM text -- go up from the first device's thread as
    their arrays (``upload_soa``), a fused set of their own, with their name keys or strand bytes when asked for.

One thread and one ``native.Context`` per device; the first exception is raised when every thread has ended.  ``junctions``,
``strandedness``, ``genecounts`` / ``exoncounts`` run on ``over_fused_sets`` or its parts, ``coverage`` / ``intronretention`` on one
context of the calling thread.  ``process.process_sites`` does not: it lays shards out with shifts, on two streams.
"""
import contextlib
import threading

from . import native


def check_fragment_source(source):
    """What pairs mates needs of a source: name keys from its decode, and the file whole on one device."""
    if not getattr(source, "mate_keys", False):
        raise native.SpliserNativeError(-1, "fragment counting needs a source decoded with name keys (DecodeOptions.mate_keys)")
    if getattr(source, "shares", None):
        raise native.SpliserNativeError(-1, "fragment counting needs the file decoded on one device: mates can lie either side of a share's cut")


def plans_of(source, devices, chroms):
    """-> [(device, [(chrom, add)])], a plan per device that has something to visit.  ``add(dr)`` adds the chromosome's reads to a
    read set of that device and returns their number; ``None``: the reads are on the host (``source.reads(chrom)``).  Waits for the
    outcome of a device decode, however it was started (``BamFile.join_decoders``: False when the host's threads have the file --
    they may still be decoding it).  ``join_decoders`` alone is the question, not ``device_decode_started() and join_decoders()`` as
    ``junctions`` once asked: the two differ only after a synchronous ``decode_on_device(ctx)`` (SAM text parsed on the GPU starts no
    decoder thread), where the longer one says "host" although the reads lie on the device -- and would send them down to the host
    and up again in every command."""
    on_device = isinstance(source, native.BamFile) and source.join_decoders()
    shares = getattr(source, "shares", None) if on_device else None
    if shares:
        plans = []
        for k, (device, names) in enumerate(shares):
            held = [c for c in chroms if c in names and source.share_ref(k, c)[0] > 0]
            plans.append((device, [(c, (lambda dr, k=k, c=c: dr.add_bam_share(source, k, c))) for c in held]))
        return plans
    if on_device:
        return [(devices[0], [(c, (lambda dr, c=c: dr.add_bam(source, c))) for c in chroms])]
    return [(devices[0], [(c, None) for c in chroms])]


def run_plans(plans, job):
    """``job(ctx, chrom, add)`` for every entry of every plan, in order: a thread and a context per plan that has an entry.  The first
    exception is raised when all threads have ended."""
    errors, lock = [], threading.Lock()

    def run(device, entries):
        try:
            with native.Context(device) as ctx:
                for chrom, add in entries:
                    job(ctx, chrom, add)
        except Exception as exc:
            with lock:
                errors.append(exc)

    workers = [threading.Thread(target=run, args=plan) for plan in plans if plan[1]]
    for w in workers:
        w.start()
    for w in workers:
        w.join()
    if errors:
        raise errors[0]


def subsample_threshold(fraction):
    """``--subsample FRAC`` -> the rule's threshold (``spl_reads_subsample``): FRAC of 2^32, rounded down; FRAC in (0, 1]."""
    fraction = float(fraction)
    if not 0.0 < fraction <= 1.0:
        raise ValueError("subsample: the fraction must be in (0, 1]")
    return int(fraction * 4294967296.0)


_kept_lock = threading.Lock()


@contextlib.contextmanager
def _selected(dr, subsample, kept, dedup=False, removed=None):
    """``dr`` itself, or -- ``subsample`` = (seed, threshold) -- the set of its reads that the rule keeps, selected on the device, or --
    ``dedup`` -- the set without its duplicate fragments (``DeviceReads.dedup``), or the second of the first: a shallower library
    is deduplicated as a shallower library would be.  What is made here is freed on the way out (None when no read is left).
    ``kept`` (or None): a list whose two entries get the reads kept by the selection and the reads they were selected from
    added; ``removed`` (or None): likewise the duplicate reads removed and the reads they were removed from."""
    if dr is None or (subsample is None and not dedup):
        yield dr
        return
    made = []
    try:
        if subsample is not None:
            sel, _ = dr.subsample(*subsample)
            made.append(sel)
            if kept is not None:
                with _kept_lock:
                    kept[0] += sel.n
                    kept[1] += dr.n
            dr = sel
        if dedup and dr.n:
            left, _ = dr.dedup()
            made.append(left)
            if removed is not None:
                with _kept_lock:
                    removed[0] += dr.n - left.n
                    removed[1] += dr.n
            if len(made) == 2:          # (the selection has served: the deduplicated set is on arrays of its own)
                made.pop(0).free()
            dr = left
        yield dr if dr.n else None
    finally:
        for s in made:
            s.free()


@contextlib.contextmanager
def fused_set(ctx, source, chrom, add, with_keys=False, with_strand=False, subsample=None, kept=None, dedup=False, removed=None):
    """One entry of a plan as a finished read set on ``ctx`` -- None when the chromosome has no read --, freed on the way out.  Reads
    on the host (``add`` None) go up as four arrays, ``with_keys`` / ``with_strand``: with their name keys / strand bytes, which the
    source must have (``DecodeOptions.mate_keys`` / ``aux_strand``).  ``subsample`` = (seed, threshold): the set handed out is the
    one ``DeviceReads.subsample`` selects from it (the source needs name keys; reads on the host go up with theirs), and ``kept`` (a list of two) gets the reads
    kept and the reads they were selected from added.  ``dedup``: the set handed out is without its duplicate fragments
    (``DeviceReads.dedup``: name keys again, and the file whole on one device -- ``check_fragment_source``), behind ``subsample`` when
    both are given; ``removed`` (a list of two) gets the reads removed and the reads they were removed from added."""
    with_keys = with_keys or subsample is not None or bool(dedup)
    if add is not None:
        with ctx.begin_reads() as dr:
            with _selected(dr.finish() if add(dr) else None, subsample, kept, dedup, removed) as out:
                yield out
        return
    rs = source.reads(chrom)
    if rs is None or not rs.n:
        yield None
        return
    if with_keys and getattr(rs, "name_key", None) is None:
        raise native.SpliserNativeError(-1, "the reads of %s were decoded without name keys (mate_keys)" % chrom)
    if with_strand and getattr(rs, "xs", None) is None:
        raise native.SpliserNativeError(-1, "%s: reads without strand bytes" % chrom)
    arrays = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, xs=rs.xs if with_strand else None, name_key=rs.name_key if with_keys else None)
    with ctx.upload_soa([arrays], [getattr(rs, "max_end", None)], with_keys=with_keys, with_strand=with_strand) as soa:
        with ctx.begin_reads() as dr:
            dr.add_soa(soa, 0)
            with _selected(dr.finish(), subsample, kept, dedup, removed) as out:
                yield out


def over_fused_sets(source, devices, chroms, visit, with_keys=False, with_strand=False, dedup=False, removed=None):
    """``visit(dr, chrom)`` for a finished, fused read set per chromosome of ``chroms`` that has a read (per piece of it, after a
    decode in shares) -- called from one thread per device, so it guards what it adds to.  ``dedup`` / ``removed``: ``fused_set``'s."""
    def job(ctx, chrom, add):
        with fused_set(ctx, source, chrom, add, with_keys, with_strand, dedup=dedup, removed=removed) as dr:
            if dr is not None:
                visit(dr, chrom)
    run_plans(plans_of(source, devices, chroms), job)
