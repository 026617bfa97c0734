#!/usr/bin/env python3
"""What `coverage --fragments` and `intronretention --fragments` cost: the fragment mark kernel beside `spl_cov_mark_kernel`, and the
fragment junction table beside `spl_junctions`, on the same reads in the same run; the marks (atomics) a read of both mark kernels,
counted exactly on the host; and both commands with and without the switch on a paired file.
Runs on the GPU box; plain Python; every run is a fresh child under a time limit of its own, and the first failure ends everything.

    tools/covfragment_rate.py [--workloads arabidopsis,human] [--human-scale 0.25] [--runs 3] [--files DIR] [--out FILE] [--tree DIR]

Per workload: the files of tools/genecount_rate.py with its synthetic annotation.  The workloads are single-end; for the kernels they
are made PAIRED in memory the way tools/mate_rate.py does, keys given directly -- within a chromosome read i and read i + GAP of
every stretch of 2 GAP reads become one fragment, flags 99 / 147 -- once with GAP = 37 (mates in one workgroup or the next) and once
with GAP = 4096 (a distant mate: what the leader's dependent loads cost when the mate's lines are nobody's neighbours).  Reported:
  (a) one child per pairing, the paired arrays: per pass a fresh read set per chromosome; `spl_coverage`, `spl_coverage_fragments`
      (the first call builds the mate table) under the library's own stopwatch (device events around the launches:
      spl_prof_report), and `spl_junctions` / `spl_junctions_fragments` with knobs 8, 70, 500000 between their own device events
      (spl_junctions_stats); summed over the chromosomes, median of --runs passes and the passes themselves.  A third child times
      `spl_junctions` on the same arrays WITHOUT keys;
  (b) the marks a read: every block of a read is two atomics in the per-read kernel; a fragment's union is counted here with numpy
      from the reads' blocks (a restatement of the rule for reads of the workload's kinds, held against the device's covered bases);
  (c) both commands with and without the switch on a PAIRED FILE: the first --paired-reads reads of the workload's first chromosome,
      paired with GAP = 37 and written with one name per fragment (the Python writer: hence a small file), a child each.
``--tree DIR``: the package of another checkout of this repository (built there) takes the runs; where its library has no
`spl_coverage_fragments` the new kernels and the switches are left out, and the yardstick kernels are timed on the same reads -- how
the numbers of two commits are set side by side."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import genecount_rate as gr  # noqa: E402  (write_annotation)
import mate_rate as mr       # noqa: E402  (paired, GAP)

MARKS = ("spl_cov_mark_kernel", "spl_cov_mark_fragments_kernel")
KNOBS = (8, 70, 500000)
GAPS = (37, 4096)


def paired(rs, k_chrom, gap):
    """``mate_rate.paired`` with a gap of the caller's."""
    old, mr.GAP = mr.GAP, gap
    try:
        return mr.paired(rs, k_chrom)
    finally:
        mr.GAP = old


def blocks_of(rs):
    """Every read's covered blocks (M, = and X; ops that abut are one block), unclipped, by numpy: -> (first[n + 1], start, end)."""
    op, ln = (rs.cigar & 15).astype(np.int64), (rs.cigar >> 4).astype(np.int64)
    n_ops = np.diff(rs.cig_off.astype(np.int64))
    owner = np.repeat(np.arange(rs.n), n_ops)
    covers = ((op == 0) | (op == 7) | (op == 8)) & (ln > 0)
    moves = (covers | (op == 2) | (op == 3)) & (ln > 0)
    step = np.where(moves, ln, 0)
    before = np.cumsum(step) - step
    base = np.zeros(rs.n + 1, np.int64)
    np.cumsum(np.bincount(owner, weights=step, minlength=rs.n).astype(np.int64), out=base[1:])
    start = rs.pos.astype(np.int64)[owner] - 1 + before - base[:-1][owner]
    s, e, o = start[covers], (start + ln)[covers], owner[covers]
    joins = np.zeros(s.shape[0], bool)
    joins[1:] = (o[1:] == o[:-1]) & (s[1:] == e[:-1])
    head = np.flatnonzero(~joins)
    tail = np.concatenate((head[1:], [s.shape[0]])) - 1
    first = np.zeros(rs.n + 1, np.int64)
    np.cumsum(np.bincount(o[head], minlength=rs.n), out=first[1:])
    return first, s[head], e[tail]


def marks_of(rs, flag, keys, gap, length):
    """-> (per-read marks, fragment marks, per-read covered bases, fragment covered bases) of one chromosome of ``length`` bases: two
    atomics a clipped block; a fragment's intervals are its two reads' clipped blocks merged where they overlap or abut."""
    first, s, e = blocks_of(rs)
    n = rs.n
    eligible = ((flag & 4) == 0) & (rs.pos >= 1) & (np.diff(first) > 0)
    s, e = np.maximum(s, 0), np.minimum(e, int(length))
    per_block = np.repeat(eligible, np.diff(first)) & (e > s)
    read_marks, read_bases = 2 * int(per_block.sum()), int((e - s)[per_block].sum())
    i = np.arange(n)
    has_mate = keys != 0
    owner_of_read = np.where(has_mate & ((i % (2 * gap)) >= gap), i - gap, i)
    owner = np.repeat(owner_of_read, np.diff(first))[per_block]
    bs, be = s[per_block], e[per_block]
    order = np.lexsort((bs, owner))
    owner, bs, be = owner[order], bs[order], be[order]
    # the running end of a fragment's intervals: a maximum restarted at every fragment (its blocks are few: a loop over their rank)
    reach = be.copy()
    same = np.zeros(owner.shape[0], bool)
    same[1:] = owner[1:] == owner[:-1]
    for _ in range(64):
        prev = np.concatenate(([0], reach[:-1]))
        new = np.where(same, np.maximum(reach, prev), reach)
        if np.array_equal(new, reach):
            break
        reach = new
    opens = np.ones(owner.shape[0], bool)
    opens[1:] = ~same[1:] | (bs[1:] > reach[:-1])
    head = np.flatnonzero(opens)
    tail = np.concatenate((head[1:], [owner.shape[0]])) - 1
    return read_marks, 2 * int(head.shape[0]), read_bases, int((reach[tail] - bs[head]).sum())


def _package(tree):
    sys.path.insert(0, tree or HERE)


def child_kernels(args):
    _package(args.tree)
    import torch  # noqa: F401  (first: one HIP runtime per process)
    from spliser_amd import native, synth
    new = hasattr(native.lib(), "spl_coverage_fragments")
    wl = synth.Workload.load(args.cache_file, args.workload) if os.path.exists(args.cache_file) else synth.Workload(args.workload, scale=args.scale, workers=16)
    lengths = [int(v) for v in wl.genome.chrom_lengths]
    arrays = []
    for k, rs in enumerate(wl.reads):
        flag, keys = paired(rs, k, args.gap) if args.gap else (rs.flag, None)
        arrays.append(native.ReadArrays(rs.pos, flag, rs.cig_off, rs.cigar, name_key=keys))
    passes, bases, pairs, rows = [], [0, 0], 0, [0, 0]
    with native.Context(0) as ctx:
        with ctx.upload_soa(arrays, with_keys=bool(args.gap)) as soa:
            for k in range(args.runs + 1):          # (pass 0 warms the device: dropped)
                native.prof_enable(True)
                bases, pairs, rows, j_ms = [0, 0], 0, [0, 0], [0.0, 0.0]
                for c in range(len(arrays)):
                    if not arrays[c].n:
                        continue
                    with ctx.begin_reads() as dr:
                        dr.add_soa(soa, c)
                        dr.finish()
                        bases[0] += dr.coverage(lengths[c])[3]["covered_bases"]
                        if new and args.gap:
                            t = dr.coverage(lengths[c], fragments=True)[3]
                            bases[1] += t["covered_bases"]
                            pairs += t["pairs"]
                        for q in range(2 if new and args.gap else 1):
                            ctx.sync()
                            ctx.kernel_timing_begin(4)
                            table = dr.junctions(0, *KNOBS, fragments=True) if q else dr.junctions(0, *KNOBS)
                            j_ms[q] += dr.junctions_stats()[1]
                            ctx.kernel_timing_collect()
                            rows[q] += int(table["count"].astype(np.int64).sum())
                report = {r["kernel"]: r for r in native.prof_report() if r["kernel"] in MARKS}
                if k:
                    p = {name: report[name]["ms"] if name in report else 0.0 for name in MARKS}
                    p.update(spl_junctions=j_ms[0], spl_junctions_fragments=j_ms[1])
                    passes.append(p)
    print("RESULT " + json.dumps({"new": new, "passes": passes, "bases": bases, "pairs": pairs, "junction_counts": rows}), flush=True)


def child_command(args):
    _package(args.tree)
    import torch  # noqa: F401
    from spliser_amd import cli, process
    logged = []

    class Tee(object):
        def write(self, text):
            logged.append(text)

        def flush(self):
            pass
    command, mode = args.child.split(":")
    argv = [command, "-B", args.prefix + ".paired.bam", "-o", args.prefix + "." + command + "." + mode] + (["-A", args.prefix + ".gtf"] if command == "intronretention" else [])
    argv += ["--fragments"] if mode == "fragments" else []
    so = sys.stdout
    t = time.perf_counter()
    sys.stdout = Tee()
    try:
        assert cli.main(argv) == 0
    finally:
        sys.stdout = so
    wall = time.perf_counter() - t
    process.wait_deferred_close()
    last = [line for line in "".join(logged).splitlines() if ".bedgraph: " in line or ".introns.tsv: " in line or line.startswith("Mates: ")]
    print("RESULT " + json.dumps({"wall_s": wall, "summary": " | ".join(x.strip() for x in last)}), flush=True)


def run_child(args, mode, prefix, extra=()):
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--prefix", prefix, "--runs", str(args.runs)] + list(extra)
    if args.tree:
        cmd += ["--tree", args.tree]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        return None, "status %d\n%s" % (p.returncode, p.stderr[-2000:])
    found = [line[7:] for line in p.stdout.splitlines() if line.startswith("RESULT ")]
    return (json.loads(found[-1]), "") if found else (None, "no RESULT line\n" + p.stdout[-2000:])


def write_paired_file(path, wl, n_reads):
    """The first reads of the first chromosome that has as many, paired with GAP = 37, a name per fragment."""
    from spliser_amd import samio
    k = next(k for k, rs in enumerate(wl.reads) if rs.n >= n_reads)
    n = n_reads - n_reads % (2 * mr.GAP)
    rs = wl.reads[k].take(0, n)
    flag, _ = mr.paired(rs, k)
    i = np.arange(n)
    leader = np.where((i % (2 * mr.GAP)) < mr.GAP, i, i - mr.GAP)
    samio.write_bam(path, wl.genome.chrom_names, wl.genome.chrom_lengths, [(wl.genome.chrom_names[k], samio.ReadSet(rs.pos, flag, rs.cig_off, rs.cigar))], with_seq=True,
                    names=[[b"f%d" % x for x in leader.tolist()]])
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="arabidopsis,human")
    ap.add_argument("--human-scale", type=float, default=0.25)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--files", default="/tmp/wl_files")
    ap.add_argument("--cache", default="/tmp/wl")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=400, help="seconds a child may take")
    ap.add_argument("--paired-reads", dest="paired_reads", type=int, default=296000, help="reads of the paired file of (c)")
    ap.add_argument("--no-commands", dest="commands", default=True, action="store_false", help="leave (c) out")
    ap.add_argument("--tree", default=None, help="another checkout of this repository whose package takes the runs")
    ap.add_argument("--child", default=None)
    ap.add_argument("--prefix", default=None)
    ap.add_argument("--workload", default=None)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--gap", type=int, default=37)
    ap.add_argument("--cache-file", dest="cache_file", default=None)
    args = ap.parse_args()
    if args.tree:
        args.tree = os.path.abspath(args.tree)
    if args.child == "kernels":
        return child_kernels(args)
    if args.child:
        return child_command(args)
    _package(args.tree)
    from spliser_amd import native, synth
    new = hasattr(native.lib(), "spl_coverage_fragments")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    os.makedirs(args.files, exist_ok=True)
    os.makedirs(args.cache, exist_ok=True)
    failed = differs = False
    for name in args.workloads.split(","):
        cfg = synth.WORKLOADS[name]
        scale = args.human_scale if name == "human" else 1.0
        prefix = os.path.join(args.files, "%s_s%g_q1" % (name, scale))
        cache = os.path.join(args.cache, "%s_s%g_seed%d.npz" % (name, scale, cfg["seed"]))
        if os.path.exists(cache) and os.path.exists(prefix + ".gtf"):          # (a workload from the cache has its reads, not its isoforms: the annotation is written once)
            wl = synth.Workload.load(cache, name)
        else:
            wl = synth.Workload(name, scale=scale, workers=16)
            wl.save(cache)
            gr.write_annotation(wl.genome, prefix + ".gtf", prefix + ".gff")
        n_reads, n_ops = sum(r.n for r in wl.reads), sum(int(r.cig_off[-1]) for r in wl.reads)
        if not os.path.exists(prefix + ".paired.bam"):
            write_paired_file(prefix + ".paired.bam", wl, args.paired_reads)
        say("%s (scale %g): %d reads, %d ops, %d chromosomes" % (name, scale, n_reads, n_ops, len(wl.genome.chrom_names)))
        host = {}
        for gap in GAPS:          # (b) on the host, from the workload's own arrays
            sums = np.zeros(4, np.int64)
            for k, rs in enumerate(wl.reads):
                if rs.n:
                    flag, keys = paired(rs, k, gap)
                    sums += marks_of(rs, flag, keys, gap, wl.genome.chrom_lengths[k])
            host[gap] = sums.tolist()
        del wl
        for gap in GAPS + (0,):
            res, why = run_child(args, "kernels", prefix, ["--workload", name, "--scale", str(scale), "--cache-file", cache, "--gap", str(gap)])
            if res is None:
                say("%s kernels (gap %d): FAILED: %s -- stopping" % (name, gap, why))
                failed = True
                break
            ms = {k: statistics.median(p[k] for p in res["passes"]) for k in res["passes"][0]}
            passes = json.dumps([{k: round(v, 3) for k, v in p.items()} for p in res["passes"]])
            if not gap:
                say("%s (a) a set WITHOUT keys, device events, ms summed over the chromosomes, median of %d passes: spl_cov_mark_kernel %.3f ms, spl_junctions %.3f ms  %s" % (
                    name, len(res["passes"]), ms[MARKS[0]], ms["spl_junctions"], passes))
                continue
            if not res["new"]:
                say("%s (a) read i with read i + %d, device events, ms summed over the chromosomes, median of %d passes (this library has no fragment kernels): spl_cov_mark_kernel %.3f ms, "
                    "spl_junctions %.3f ms  %s" % (name, gap, len(res["passes"]), ms[MARKS[0]], ms["spl_junctions"], passes))
                continue
            rm, fm, rb, fb = host[gap]
            same = res["bases"] == [rb, fb]
            say("%s, read i with read i + %d: %d pairs whose union was taken; covered bases per read %d, per fragment %d; the device's equal the host restatement's: %s; junction counts per read %d, "
                "per fragment %d" % (name, gap, res["pairs"], rb, fb, same, res["junction_counts"][0], res["junction_counts"][1]))
            if not same:          # (said, and the run ends with status 1; the timings are still taken)
                say("%s: the device's covered bases are %s" % (name, res["bases"]))
                differs = True
            say("%s (a) device events, ms summed over the chromosomes, median of %d passes: spl_cov_mark_fragments_kernel %.3f ms, spl_cov_mark_kernel %.3f ms (%.2f x); spl_junctions_fragments %.3f ms, "
                "spl_junctions %.3f ms (%.2f x)  %s" % (name, len(res["passes"]), ms[MARKS[1]], ms[MARKS[0]], ms[MARKS[1]] / ms[MARKS[0]] if ms[MARKS[0]] else 0.0, ms["spl_junctions_fragments"],
                                                       ms["spl_junctions"], ms["spl_junctions_fragments"] / ms["spl_junctions"] if ms["spl_junctions"] else 0.0, passes))
            say("%s (b) marks (atomics): per read %d = %.4f a read; per fragment %d = %.4f a read" % (name, rm, rm / float(n_reads), fm, fm / float(n_reads)))
        if failed:
            break
        if not args.commands:
            continue
        modes = [c + ":" + m for c in ("coverage", "intronretention") for m in (("reads", "fragments") if new else ("reads",))]
        walls, summary = {m: [] for m in modes}, {}
        for k in range(args.runs + 1):          # (round 0 warms the page cache and the device: dropped)
            for mode in modes:
                r, why = run_child(args, mode, prefix)
                if r is None:
                    say("%s %s run %d: FAILED: %s -- stopping" % (name, mode, k, why))
                    failed = True
                    break
                if k:
                    walls[mode].append(r["wall_s"])
                    summary[mode] = r["summary"]
            if failed:
                break
        if failed:
            break
        for mode in modes:
            w = walls[mode]
            command, m = mode.split(":")
            say("%s (c) `%s%s` on the paired file: median %.4f s, min %.4f, max %.4f  %s" % (name, command, " --fragments" if m == "fragments" else "", statistics.median(w), min(w), max(w),
                                                                                         ["%.4f" % x for x in w]))
            say("    " + summary[mode])
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 1 if failed or differs else 0


if __name__ == "__main__":
    sys.exit(main())
