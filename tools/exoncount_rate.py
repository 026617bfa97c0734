#!/usr/bin/env python3
"""What `exoncounts` costs: its kernel beside `spl_gene_count` on the same reads in the same run (that kernel is the yardstick: this
work leaves it as it was), the 64-bit adds its commit issues, its bytes floor, and the command beside `genecounts` on the same file.
Runs on the GPU box; plain Python; every run is a fresh child under a time limit of its own, and the first failure ends everything.

    tools/exoncount_rate.py [--workloads arabidopsis,human] [--human-scale 0.25] [--runs 3] [--files DIR] [--out FILE]

Per workload: the two files of tools/genecount_rate.py with the same synthetic annotation (its ``write_annotation``).  Reported:
  (a) one child decodes the file on the device and runs, per chromosome on the same fused set, `spl_gene_count` with its gene map
      and `spl_exon_count` with its bin map -- a warm-up pass, then --runs passes under the library's own stopwatch (device events
      around the launches: spl_prof_report), summed over the chromosomes, median of the passes and their spread;
  (b) the 64-bit adds a read, computed here exactly from every read's hit list (a numpy restatement of the rule over the workload's
      arrays, held against the device's counts) under the commit's own round rule -- in round j every lane of a wave of 64 reads in
      file order offers its j-th bin, and every run of equal bins in lane order is one add -- beside the naive count of one add per
      (read, bin);
  (c) the bytes floor (10 B a read, 4 B an op) and the share of 8 TB/s the kernel reaches;
  (d) the command's wall clock beside `genecounts`, a child each."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import genecount_rate as gr  # noqa: E402  (write_annotation, the bytes floor's constants)

KERNELS = ("spl_exon_count_kernel", "spl_gene_count_kernel")
SHARED = 0xFFFFFFFF


def hits_of(rs, bin_map, bin_gene):
    """Every read's verdict (0 counted, -1 no feature, -2 ambiguous, -3 not counted) and the hit lists of the counted reads, in
    numpy: -> (verdict[n], first[n + 1], bins) -- read r's bins are bins[first[r]:first[r + 1]], in the order of their stretches.
    Covering ops are taken one by one: ops that abut overlap the same stretches as their union, and a stretch is taken once."""
    start, code = bin_map[0].astype(np.int64), bin_map[1].astype(np.int64)
    n = rs.n
    off = rs.cig_off.astype(np.int64)
    n_ops = np.diff(off)
    op, length = (rs.cigar & 15).astype(np.int64), (rs.cigar >> 4).astype(np.int64)
    read_of = np.repeat(np.arange(n), n_ops)
    consumes = (op == 0) | (op == 2) | (op == 3) | (op == 7) | (op == 8)
    adv = np.where(consumes, length, 0)
    before = np.cumsum(adv) - adv
    if len(read_of):
        before -= before[np.minimum(off[:-1], len(before) - 1)][read_of]          # reference bases in front of the op, within its read
    eligible = ((rs.flag & (0x4 | 0x100 | 0x200 | 0x800)) == 0) & (rs.pos >= 1) & (n_ops >= 1)
    covers = ((op == 0) | (op == 7) | (op == 8)) & (length > 0) & eligible[read_of]
    s = (rs.pos.astype(np.int64)[read_of] - 1 + before)[covers]
    e = s + length[covers]
    who = read_of[covers]
    k0 = np.maximum(np.searchsorted(start, s, "right") - 1, 0)
    k1 = np.searchsorted(start, e - 1, "right") - 1          # (-1: the block lies below the first entry)
    span = np.maximum(k1 - k0 + 1, 0)
    r = np.repeat(who, span)
    k = np.repeat(k0 - (np.cumsum(span) - span), span) + np.arange(int(span.sum()))
    new = np.ones(len(r), bool)
    new[1:] = (r[1:] != r[:-1]) | (k[1:] != k[:-1])          # (reads, ops and stretches all ascend: a stretch hit again follows itself)
    c = code[k] if len(code) else np.zeros(0, np.int64)
    keep = new & (c != 0)
    r, c = r[keep], c[keep]
    shared = np.zeros(n, bool)
    shared[r[c == SHARED]] = True
    own = c != SHARED
    gene = np.zeros(len(c), np.int64)
    gene[own] = bin_gene.astype(np.int64)[c[own] - 1]
    low, high = np.full(n, np.iinfo(np.int64).max), np.full(n, -1, np.int64)
    np.minimum.at(low, r[own], gene[own])
    np.maximum.at(high, r[own], gene[own])
    verdict = np.where(~eligible, -3, np.where(shared | ((high >= 0) & (low != high)), -2, np.where(high >= 0, 0, -1)))
    counted = verdict[r] == 0
    r, c = r[counted], c[counted]
    first = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=first[1:])
    return verdict, first, c - 1


def round_adds(first, bins):
    """The adds of the commit's round rule over these reads in this order, waves of 64: the j-th bin of a read is an add unless the
    read before it in its wave has a j-th bin and it is the same."""
    n = len(first) - 1
    hits = np.diff(first)
    r = np.repeat(np.arange(n), hits)
    j = np.arange(len(bins)) - first[r]
    has_before = (r % 64 != 0) & (j < hits[np.maximum(r - 1, 0)])
    before = bins[np.minimum(first[np.maximum(r - 1, 0)] + j, max(len(bins) - 1, 0))] if len(bins) else bins
    return int((~(has_before & (before == bins))).sum())


def child_kernels(args):
    sys.path.insert(0, HERE)
    import torch  # noqa: F401  (first: one HIP runtime per process)
    from spliser_amd import exoncounts as xc, genecounts as gc, native, process
    quiet = lambda m: None
    source = process.open_and_decode(args.prefix + ".bam", (0,), True, 16, process.DecodeOptions(), log=quiet)
    try:
        source.wait_all()
        assert source.join_decoders(), source.decline_reason()
        chroms = list(source.ref_names)
        features = gc.read_features(args.prefix + ".gtf")
        maps = gc.maps_of(features, chroms)
        bins = xc.Bins(features)
        n_genes = len(features.ids)
        nothing = (None, None, np.zeros(0, np.uint32))
        passes, per_bin, verdicts = [], None, None
        with native.Context(0) as ctx:
            for k in range(args.runs + 1):          # (pass 0 warms the device: dropped)
                native.prof_enable(True)
                genes, per_bin, verdicts = np.zeros(n_genes + 3, np.int64), {}, np.zeros(4, np.int64)
                for chrom in chroms:
                    with ctx.begin_reads() as dr:
                        if not dr.add_bam(source, chrom):
                            continue
                        dr.finish()
                        dr.gene_counts(n_genes, *maps.get(chrom, (None, None)), out=genes)
                        a, b, bin_gene = bins.by_chrom.get(chrom, nothing)
                        t = dr.exon_counts(bin_gene, a, b)
                        per_bin[chrom] = t[:-4].tolist()
                        verdicts += t[-4:]
                report = {r["kernel"]: r for r in native.prof_report() if r["kernel"] in KERNELS}
                if k:
                    passes.append({name: {"ms": r["ms"], "bytes": r["bytes"], "calls": r["calls"]} for name, r in report.items()})
    finally:
        source.close()
    print("RESULT " + json.dumps({"passes": passes, "per_bin": per_bin, "verdicts": verdicts.tolist(), "genes": genes.tolist()}), flush=True)


def child_command(args):
    sys.path.insert(0, HERE)
    import torch  # noqa: F401
    from spliser_amd import cli, process
    logged = []

    class Tee(object):
        def write(self, text):
            logged.append(text)

        def flush(self):
            pass
    argv = [args.child, "-B", args.prefix + ".bam", "-A", args.prefix + ".gtf", "-o", args.prefix + ".rate"]
    so = sys.stdout
    t = time.perf_counter()
    sys.stdout = Tee()
    try:
        assert cli.main(argv) == 0
    finally:
        sys.stdout = so
    wall = time.perf_counter() - t
    process.wait_deferred_close()
    found = re.search(r"\(read in ([0-9.]+) s\)", "".join(logged))
    last = [line for line in "".join(logged).splitlines() if "counts.tsv: " in line]
    print("RESULT " + json.dumps({"wall_s": wall, "reader_s": float(found.group(1)) if found else None, "summary": last[-1].strip() if last else ""}), flush=True)


def run_child(args, mode, prefix):
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--prefix", prefix, "--runs", str(args.runs)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        return None, "status %d\n%s" % (p.returncode, p.stderr[-2000:])
    found = [line[7:] for line in p.stdout.splitlines() if line.startswith("RESULT ")]
    return (json.loads(found[-1]), "") if found else (None, "no RESULT line\n" + p.stdout[-2000:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="arabidopsis,human")
    ap.add_argument("--human-scale", type=float, default=0.25)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--files", default="/tmp/wl_files")
    ap.add_argument("--cache", default="/tmp/wl")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--child", default=None)
    ap.add_argument("--prefix", default=None)
    args = ap.parse_args()
    if args.child == "kernels":
        return child_kernels(args)
    if args.child:
        return child_command(args)
    sys.path.insert(0, HERE)
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
        wl = synth.Workload.load(cache, name) if os.path.exists(cache) else synth.Workload(name, scale=scale, workers=16)
        n_reads, n_ops = sum(r.n for r in wl.reads), sum(int(r.cig_off[-1]) for r in wl.reads)
        if not os.path.exists(prefix + ".bam"):
            native.write_bam(prefix + ".bam", wl.genome.chrom_names, wl.genome.chrom_lengths, wl.reads, level=1, threads=16, seq_mode=1)
        gr.write_annotation(wl.genome, prefix + ".gtf", prefix + ".gff")
        say("%s (scale %g): %d reads, %d ops, %d chromosomes, %.1f MB BAM, %.1f MB GTF" % (name, scale, n_reads, n_ops, len(wl.genome.chrom_names), os.path.getsize(prefix + ".bam") / 1e6,
                                                                                         os.path.getsize(prefix + ".gtf") / 1e6))
        # (b) on the host, from the workload's own arrays: every read's verdict and hit list, the counts, the adds of the round rule
        features = gc.read_features(prefix + ".gtf")
        t = time.perf_counter()
        bins = xc.Bins(features)
        cut_s = time.perf_counter() - t
        host_bins, host_verdicts, adds, naive, most = {}, np.zeros(4, np.int64), 0, 0, 0
        empty = (np.zeros(0, np.int32), np.zeros(0, np.uint32))
        for chrom, rs in zip(wl.genome.chrom_names, wl.reads):
            a, _, bin_gene = bins.by_chrom.get(chrom, (empty, None, np.zeros(0, np.uint32)))
            verdict, first, hit = hits_of(rs, a, bin_gene)
            host_verdicts += np.bincount(-verdict, minlength=4)
            if rs.n:
                host_bins[chrom] = np.bincount(hit, minlength=bin_gene.shape[0]).tolist()
            adds += round_adds(first, hit)
            naive += len(hit)
            most = max(most, int(np.diff(first).max()) if rs.n else 0)
        del wl
        say("%s annotation: %d genes, %d bins, %d map entries; cut into bins in %.3f s" % (name, len(features.ids), bins.n, sum(m[0][0].shape[0] for m in bins.by_chrom.values()), cut_s))
        res, why = run_child(args, "kernels", prefix)
        if res is None:
            say("%s kernels: FAILED: %s -- stopping" % (name, why))
            failed = True
            break
        same = res["verdicts"] == host_verdicts.tolist() and res["per_bin"] == host_bins
        gene_same = res["verdicts"] == [sum(res["genes"][:-3])] + res["genes"][-3:]
        say("%s counts: %d counted, %d no feature, %d ambiguous, %d not counted; the device's bins and verdicts equal the host restatement's: %s; its verdicts equal spl_gene_count's: %s" % (
            (name,) + tuple(int(v) for v in host_verdicts) + (same, gene_same)))
        if not (same and gene_same):
            failed = True
            break
        ms = {k: statistics.median(p[k]["ms"] for p in res["passes"]) for k in KERNELS}
        say("%s (a) device events, ms summed over the chromosomes, median of %d passes: spl_exon_count %.3f ms, spl_gene_count %.3f ms: %.2f x  %s" % (
            name, len(res["passes"]), ms[KERNELS[0]], ms[KERNELS[1]], ms[KERNELS[0]] / ms[KERNELS[1]] if ms[KERNELS[1]] else 0.0,
            json.dumps([{k: round(p[k]["ms"], 3) for k in KERNELS} for p in res["passes"]])))
        counted = int(host_verdicts[0])
        say("%s (b) 64-bit adds: %d under the round rule for %d reads = %.4f a read (%.4f a counted read); one per (read, bin) would be %d = %.4f a read; a counted read has %.3f bins, at most %d" % (
            name, adds, n_reads, adds / float(n_reads), adds / float(max(counted, 1)), naive, naive / float(n_reads), naive / float(max(counted, 1)), most))
        floor_bytes = 10.0 * n_reads + 4.0 * n_ops
        say("%s (c) bytes floor: 10 B a read + 4 B an op = %.3f GB = %.3f ms at 8 TB/s; the kernel takes %.3f ms: %.1f %% of 8 TB/s, %.2f G reads/s" % (
            name, floor_bytes / 1e9, floor_bytes / gr.HBM_BYTES_PER_S * 1e3, ms[KERNELS[0]], 100.0 * floor_bytes / gr.HBM_BYTES_PER_S / (ms[KERNELS[0]] / 1e3), n_reads / (ms[KERNELS[0]] / 1e3) / 1e9))
        walls, summary = {"exoncounts": [], "genecounts": []}, ""
        for k in range(args.runs + 1):          # (round 0 warms the page cache and the device: dropped)
            for mode in ("exoncounts", "genecounts"):
                r, why = run_child(args, mode, prefix)
                if r is None:
                    say("%s %s run %d: FAILED: %s -- stopping" % (name, mode, k, why))
                    failed = True
                    break
                if k:
                    walls[mode].append(r["wall_s"])
                    if mode == "exoncounts":
                        summary = r["summary"]
            if failed:
                break
        if failed:
            break
        for mode in ("exoncounts", "genecounts"):
            w = walls[mode]
            say("%s (d) `%s`: median %.4f s, min %.4f, max %.4f  %s" % (name, mode, statistics.median(w), min(w), max(w), ["%.4f" % x for x in w]))
        say("    " + summary)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
