#!/usr/bin/env python3
"""What `exoncounts --countReadPairs` costs: its kernel beside `spl_exon_count` and beside `spl_gene_count_fragments` on the same
reads in the same run (those two kernels are the yardsticks: this work leaves them as they were), the 64-bit adds its commit issues,
its bytes floor, and the command with and without the switch on a paired file.
Runs on the GPU box; plain Python; every run is a fresh child under a time limit of its own, and the first failure ends everything.

    tools/exonfragment_rate.py [--workloads arabidopsis,human] [--human-scale 0.25] [--runs 3] [--files DIR] [--out FILE] [--tree DIR]

Per workload: the two files of tools/genecount_rate.py with the same synthetic annotation (its ``write_annotation``).  The workloads
are single-end; for the kernels they are made PAIRED in memory the way tools/mate_rate.py does (its ``paired``: within a chromosome
read i and read i + 37 in file order become one fragment, flags 99 / 147, one key for both, given directly) and go up with their keys
(``upload_soa``).  Reported:
  (a) one child, the paired arrays: per pass a fresh read set per chromosome, `spl_exon_count`, `spl_gene_count_fragments` (which
      builds the mate table) and `spl_exon_count_fragments` under the library's own stopwatch (device events around the launches:
      spl_prof_report), summed over the chromosomes, median of --runs passes and the passes themselves;
  (b) the 64-bit adds a read, computed here exactly from every fragment's merged list (tools/exoncount_rate.py's numpy restatement
      of the per-read rule, its lists united per fragment here, held against the device's counts) under the commit's own round rule
      -- in round j every lane of a wave of 64 reads in file order offers its j-th bin, a silent lane offers nothing, and every run
      of equal bins in lane order is one add -- beside one add per (fragment, bin), and beside the per-read kernel's adds on the
      same reads;
  (c) the bytes floor (14 B a read, 4 B an op) and the share of 8 TB/s the kernel reaches;
  (d) the command with and without the switch on a PAIRED FILE: the first --paired-reads reads of the workload's first chromosome,
      paired the same way and written with one name per fragment (the Python writer: hence a small file), a child each.
``--tree DIR``: the package of another checkout of this repository (built there) takes the runs; where its library has no
`spl_exon_count_fragments` the new kernel and the switch are left out, and the two yardstick kernels are timed on the same reads --
how the numbers of two commits are set side by side."""
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
import exoncount_rate as xr  # noqa: E402  (hits_of, round_adds)
import genecount_rate as gr  # noqa: E402  (write_annotation, the bytes floor's constants)
import mate_rate as mr       # noqa: E402  (paired, GAP)

KERNELS = ("spl_exon_count_fragments_kernel", "spl_exon_count_kernel", "spl_gene_count_fragments_kernel")


def fragment_lists(flag, keys, verdict, first, hit, bin_gene):
    """The per-read verdicts and hit lists of ``exoncount_rate.hits_of`` united per fragment of ``mate_rate.paired``'s pairing
    (read i of a stretch's first half leads, read i + GAP is silent; a read with key 0 is alone): -> (verdict[n] with -4 for a
    silent read, first[n + 1], bins) -- the leader's distinct bins ascending, nothing for any other verdict."""
    n = len(flag)
    i = np.arange(n)
    has_mate = keys != 0
    silent = has_mate & ((i % (2 * mr.GAP)) >= mr.GAP)
    lead = ~silent
    mate = np.where(has_mate & lead, i + mr.GAP, i)          # (a read alone: itself)
    hits = np.diff(first)
    gene = np.full(n, -1, np.int64)                          # a counted read's gene
    counted = verdict == 0
    gene[counted] = bin_gene.astype(np.int64)[hit[first[:-1][counted]]]
    v1, v2, g1, g2 = verdict, verdict[mate], gene, gene[mate]
    ambiguous = (v1 == -2) | (v2 == -2) | ((g1 >= 0) & (g2 >= 0) & (g1 != g2))
    out = np.where(silent, -4, np.where(verdict == -3, -3, np.where(ambiguous, -2, np.where((g1 >= 0) | (g2 >= 0), 0, -1))))
    # the bins of the counted fragments: both reads' lists under the leader's index, each (leader, bin) once
    owner = np.where(silent, i - mr.GAP, i)
    r = np.repeat(owner, hits)
    keep = out[r] == 0
    pair = np.unique(np.stack((r[keep], hit[keep]), axis=1), axis=0) if keep.any() else np.zeros((0, 2), np.int64)
    merged_first = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(pair[:, 0], minlength=n), out=merged_first[1:])
    return out, merged_first, pair[:, 1]


def _package(tree):
    sys.path.insert(0, tree or HERE)


def child_kernels(args):
    _package(args.tree)
    import torch  # noqa: F401  (first: one HIP runtime per process)
    from spliser_amd import exoncounts as xc, genecounts as gc, native, synth
    new = hasattr(native.lib(), "spl_exon_count_fragments")
    wl = synth.Workload.load(args.cache_file, args.workload) if os.path.exists(args.cache_file) else synth.Workload(args.workload, scale=args.scale, workers=16)
    chroms = list(wl.genome.chrom_names)
    features = gc.read_features(args.prefix + ".gtf")
    maps = gc.maps_of(features, chroms)
    bins = xc.Bins(features)
    n_genes = len(features.ids)
    nothing = (None, None, np.zeros(0, np.uint32))
    arrays = []
    for k, rs in enumerate(wl.reads):
        flag, keys = mr.paired(rs, k)
        arrays.append(native.ReadArrays(rs.pos, flag, rs.cig_off, rs.cigar, name_key=keys))
    passes, per_bin, verdicts, genes, pairs = [], {}, None, None, 0
    with native.Context(0) as ctx:
        with ctx.upload_soa(arrays, with_keys=True) as soa:
            for k in range(args.runs + 1):          # (pass 0 warms the device: dropped)
                native.prof_enable(True)
                genes, per_bin, verdicts, pairs = np.zeros(n_genes + 3, np.int64), {}, np.zeros(4, np.int64), 0
                for c, chrom in enumerate(chroms):
                    if not arrays[c].n:
                        continue
                    with ctx.begin_reads() as dr:
                        dr.add_soa(soa, c)
                        dr.finish()
                        a, b, bin_gene = bins.by_chrom.get(chrom, nothing)
                        dr.exon_counts(bin_gene, a, b)
                        dr.gene_counts(n_genes, *maps.get(chrom, (None, None)), out=genes, fragments=True)
                        pairs += dr.mate_table(0)[1]["paired"] // 2
                        if new:
                            t = dr.exon_counts(bin_gene, a, b, fragments=True)
                            per_bin[chrom] = t[:-4].tolist()
                            verdicts += t[-4:]
                report = {r["kernel"]: r for r in native.prof_report() if r["kernel"] in KERNELS}
                if k:
                    passes.append({name: report[name]["ms"] if name in report else 0.0 for name in KERNELS})
    print("RESULT " + json.dumps({"new": new, "passes": passes, "per_bin": per_bin, "verdicts": verdicts.tolist(), "genes": genes.tolist(), "pairs": pairs}), flush=True)


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
    argv = ["exoncounts", "-B", args.prefix + ".paired.bam", "-A", args.prefix + ".gtf", "-o", args.prefix + "." + args.child] + (["--countReadPairs"] if args.child == "pairs" else [])
    so = sys.stdout
    t = time.perf_counter()
    sys.stdout = Tee()
    try:
        assert cli.main(argv) == 0
    finally:
        sys.stdout = so
    wall = time.perf_counter() - t
    process.wait_deferred_close()
    last = [line for line in "".join(logged).splitlines() if ".exoncounts.tsv: " in line or line.startswith("  mates: ")]
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
    """The first reads of the first chromosome that has as many, paired as ``mate_rate.paired`` pairs them, a name per fragment."""
    from spliser_amd import samio
    k = next(k for k, rs in enumerate(wl.reads) if rs.n >= n_reads)
    n = n_reads - n_reads % (2 * mr.GAP)
    rs = wl.reads[k].take(0, n)
    flag, _ = mr.paired(rs, k)
    i = np.arange(n)
    leader = np.where((i % (2 * mr.GAP)) < mr.GAP, i, i - mr.GAP)
    paired_rs = samio.ReadSet(rs.pos, flag, rs.cig_off, rs.cigar)
    samio.write_bam(path, wl.genome.chrom_names, wl.genome.chrom_lengths, [(wl.genome.chrom_names[k], paired_rs)], with_seq=True, names=[[b"f%d" % x for x in leader.tolist()]])
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
    ap.add_argument("--paired-reads", dest="paired_reads", type=int, default=296000, help="reads of the paired file of (d)")
    ap.add_argument("--tree", default=None, help="another checkout of this repository whose package takes the runs")
    ap.add_argument("--child", default=None)
    ap.add_argument("--prefix", default=None)
    ap.add_argument("--workload", default=None)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--cache-file", dest="cache_file", default=None)
    args = ap.parse_args()
    if args.tree:
        args.tree = os.path.abspath(args.tree)
    if args.child == "kernels":
        return child_kernels(args)
    if args.child:
        return child_command(args)
    _package(args.tree)
    from spliser_amd import exoncounts as xc, genecounts as gc, native, synth
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    os.makedirs(args.files, exist_ok=True)
    os.makedirs(args.cache, exist_ok=True)
    failed = False
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
        say("%s (scale %g): %d reads, %d ops, %d chromosomes; paired in memory: read i with read i + %d" % (name, scale, n_reads, n_ops, len(wl.genome.chrom_names), mr.GAP))
        # (b) on the host, from the workload's own arrays: every fragment's verdict and merged list, the counts, the adds of the round rule
        features = gc.read_features(prefix + ".gtf")
        bins = xc.Bins(features)
        host_bins, host_verdicts, adds, naive, most, read_adds, read_naive, n_pairs = {}, np.zeros(4, np.int64), 0, 0, 0, 0, 0, 0
        empty = (np.zeros(0, np.int32), np.zeros(0, np.uint32))
        for k, (chrom, rs) in enumerate(zip(wl.genome.chrom_names, wl.reads)):
            a, _, bin_gene = bins.by_chrom.get(chrom, (empty, None, np.zeros(0, np.uint32)))
            flag, keys = mr.paired(rs, k)
            verdict, first, hit = xr.hits_of(type(rs)(rs.pos, flag, rs.cig_off, rs.cigar), a, bin_gene)
            read_adds += xr.round_adds(first, hit)
            read_naive += len(hit)
            verdict, first, hit = fragment_lists(flag, keys, verdict, first, hit, bin_gene)
            n_pairs += int((verdict == -4).sum())
            host_verdicts += np.bincount(-verdict[verdict != -4], minlength=4)
            if rs.n:
                host_bins[chrom] = np.bincount(hit, minlength=bin_gene.shape[0]).tolist()
            adds += xr.round_adds(first, hit)
            naive += len(hit)
            most = max(most, int(np.diff(first).max()) if rs.n else 0)
        del wl
        res, why = run_child(args, "kernels", prefix, ["--workload", name, "--scale", str(scale), "--cache-file", cache])
        if res is None:
            say("%s kernels: FAILED: %s -- stopping" % (name, why))
            failed = True
            break
        ms = {k: statistics.median(p[k] for p in res["passes"]) for k in KERNELS}
        passes = json.dumps([{k: round(v, 3) for k, v in p.items()} for p in res["passes"]])
        if not res["new"]:
            say("%s (a) device events, ms summed over the chromosomes, median of %d passes (this library has no fragment kernel for exon bins): spl_exon_count %.3f ms, spl_gene_count_fragments %.3f ms  %s" % (
                name, len(res["passes"]), ms[KERNELS[1]], ms[KERNELS[2]], passes))
            continue
        same = res["verdicts"] == host_verdicts.tolist() and res["per_bin"] == host_bins and res["pairs"] == n_pairs
        gene_same = res["verdicts"] == [sum(res["genes"][:-3])] + res["genes"][-3:]
        say("%s counts: %d pairs; %d fragments counted, %d no feature, %d ambiguous, %d not counted; the device's bins and verdicts equal the host restatement's: %s; its verdicts equal spl_gene_count_fragments': %s" % (
            (name, n_pairs) + tuple(int(v) for v in host_verdicts) + (same, gene_same)))
        if not (same and gene_same):
            failed = True
            break
        say("%s (a) device events, ms summed over the chromosomes, median of %d passes: spl_exon_count_fragments %.3f ms, spl_exon_count %.3f ms (%.2f x), spl_gene_count_fragments %.3f ms (%.2f x)  %s" % (
            name, len(res["passes"]), ms[KERNELS[0]], ms[KERNELS[1]], ms[KERNELS[0]] / ms[KERNELS[1]] if ms[KERNELS[1]] else 0.0, ms[KERNELS[2]],
            ms[KERNELS[0]] / ms[KERNELS[2]] if ms[KERNELS[2]] else 0.0, passes))
        counted = int(host_verdicts[0])
        say("%s (b) 64-bit adds: %d under the round rule for %d reads = %.4f a read (%.4f a counted fragment); one per (fragment, bin) would be %d = %.4f a read; a counted fragment has %.3f bins, at most %d; "
            "the per-read kernel on the same reads: %d adds = %.4f a read, one per (read, bin) %d" % (
                name, adds, n_reads, adds / float(n_reads), adds / float(max(counted, 1)), naive, naive / float(n_reads), naive / float(max(counted, 1)), most, read_adds,
                read_adds / float(n_reads), read_naive))
        floor_bytes = 14.0 * n_reads + 4.0 * n_ops
        say("%s (c) bytes floor: 14 B a read + 4 B an op = %.3f GB = %.3f ms at 8 TB/s; the kernel takes %.3f ms: %.1f %% of 8 TB/s, %.2f G reads/s" % (
            name, floor_bytes / 1e9, floor_bytes / gr.HBM_BYTES_PER_S * 1e3, ms[KERNELS[0]], 100.0 * floor_bytes / gr.HBM_BYTES_PER_S / (ms[KERNELS[0]] / 1e3), n_reads / (ms[KERNELS[0]] / 1e3) / 1e9))
        walls, summary = {"reads": [], "pairs": []}, {}
        for k in range(args.runs + 1):          # (round 0 warms the page cache and the device: dropped)
            for mode in ("reads", "pairs"):
                r, why = run_child(args, mode, prefix)
                if r is None:
                    say("%s exoncounts (%s) run %d: FAILED: %s -- stopping" % (name, mode, k, why))
                    failed = True
                    break
                if k:
                    walls[mode].append(r["wall_s"])
                    summary[mode] = r["summary"]
            if failed:
                break
        if failed:
            break
        for mode in ("reads", "pairs"):
            w = walls[mode]
            say("%s (d) `exoncounts%s` on the paired file: median %.4f s, min %.4f, max %.4f  %s" % (name, " --countReadPairs" if mode == "pairs" else "", statistics.median(w), min(w), max(w),
                                                                                                   ["%.4f" % x for x in w]))
            say("    " + summary[mode])
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
