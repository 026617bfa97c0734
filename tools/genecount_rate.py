#!/usr/bin/env python3
"""What `genecounts` costs: its kernel beside `spl_strand_tally` on the same reads in the same run, the atomics its histogram issues,
its bytes floor, and the command beside `strandedness -A` on the same file.
Runs on the GPU box; plain Python; every run is a fresh child under a time limit of its own, and the first failure ends everything.

    tools/genecount_rate.py [--workloads arabidopsis,human] [--human-scale 0.25] [--runs 3] [--files DIR] [--out FILE]

Per workload (``synth.Workload``: the 20 M-read A. thaliana-shaped sample and the 50 M-read quarter of the human-shaped one that
tools/coverage_rate.py uses, written once as a seq-like BAM).  The annotation is synthetic: ``synth.py``'s genes, a GTF with an
``exon`` line per exon of every isoform (and the genes as a GFF for `strandedness -A`).  Reported:
  (a) one child decodes the file on the device and runs, per chromosome on the same fused set, `spl_strand_tally` with its cover
      map and `spl_gene_count` with its gene map -- a warm-up pass, then --runs passes under the library's own stopwatch (device
      events around the launches: spl_prof_report), summed over the chromosomes, median of the passes;
  (b) the global atomics the histogram issues per read, computed here exactly from every read's result (a numpy restatement of
      the rule over the workload's arrays, held against the device's counts): run heads per wave of 64 reads in file order, per
      chromosome -- against the one per read a naive histogram would issue;
  (c) the bytes floor (10 B a read, 4 B an op) and the share of 8 TB/s the kernel reaches;
  (d) the command's wall clock beside `strandedness -A`, a child each, and the annotation reader's share of it."""
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
HBM_BYTES_PER_S = 8.0e12
KERNELS = ("spl_gene_count_kernel", "spl_strand_tally_kernel")


def write_annotation(genome, gtf, gff):
    """An ``exon`` line per exon of every isoform (gene_id = the gene's name), and the genes as the GFF `strandedness -A` reads."""
    from spliser_amd import synth
    synth.write_gff(gff, genome)
    ex_iso = np.repeat(np.arange(len(genome.iso_off) - 1), np.diff(genome.iso_off))
    gene = np.asarray(genome.iso_gene)[ex_iso]
    with open(gtf, "w") as fh:
        for e in range(len(ex_iso)):
            g = int(gene[e])
            fh.write('%s\tsynth\texon\t%d\t%d\t.\t%s\t.\tgene_id "%s"; transcript_id "%s.%d";\n' % (
                genome.chrom_names[int(genome.gene_chrom[g])], int(genome.ex_start[e]), int(genome.ex_end[e]), chr(int(genome.gene_strand[g])), genome.gene_names[g],
                genome.gene_names[g], int(ex_iso[e])))


def results_of(rs, gene_map):
    """Every read's result by the rule, in numpy: the gene's index, -1 no feature, -2 ambiguous, -3 not counted.  Covering ops are
    taken one by one (ops that abut overlap the same stretches as their union)."""
    start, code = gene_map[0].astype(np.int64), gene_map[1].astype(np.int64)
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
    covers = ((op == 0) | (op == 7) | (op == 8)) & (length > 0)
    s = (rs.pos.astype(np.int64)[read_of] - 1 + before)[covers]
    e = s + length[covers]
    who = read_of[covers]
    k0 = np.searchsorted(start, s, "right") - 1
    k1 = np.searchsorted(start, e - 1, "right") - 1
    many = np.zeros(n, bool)
    low, high = np.full(n, np.iinfo(np.int64).max), np.zeros(n, np.int64)
    live = np.arange(len(s))
    d = 0
    while len(live):
        k = k0[live] + d
        c = np.where(k >= 0, code[np.maximum(k, 0)], 0) if len(code) else np.zeros(len(live), np.int64)
        r = who[live]
        np.logical_or.at(many, r[c == 0xFFFFFFFF], True)
        one = (c > 0) & (c != 0xFFFFFFFF)
        np.minimum.at(low, r[one], c[one])
        np.maximum.at(high, r[one], c[one])
        d += 1
        live = live[k0[live] + d <= k1[live]]
    out = np.where(many | ((high > 0) & (low != high)), -2, np.where(high > 0, high - 1, -1))
    eligible = ((rs.flag & (0x4 | 0x100 | 0x200 | 0x800)) == 0) & (rs.pos >= 1) & (n_ops >= 1)
    return np.where(eligible, out, -3)


def run_heads(results):
    """The adds of a wave-by-wave count of runs: a lane is a head when it is the wave's first or its result differs from the lane's
    before it; heads whose result is a gene add."""
    head = np.ones(len(results), bool)
    head[1:] = results[1:] != results[:-1]
    head |= (np.arange(len(results)) % 64) == 0
    return int((head & (results >= 0)).sum())


def child_kernels(args):
    sys.path.insert(0, HERE)
    import torch  # noqa: F401  (first: one HIP runtime per process)
    from spliser_amd import genecounts as gc, native, process, sites, strandedness as sd
    quiet = lambda m: None
    source = process.open_and_decode(args.prefix + ".bam", (0,), True, 16, process.DecodeOptions(), log=quiet)
    try:
        source.wait_all()
        assert source.join_decoders(), source.decline_reason()
        chroms = list(source.ref_names)
        features = gc.read_features(args.prefix + ".gtf")
        maps = gc.maps_of(features, chroms)
        covers = sd.covers_of(sites.GeneBins.from_annotation(args.prefix + ".gff", "gene", "All", log=quiet), chroms)
        n_genes = len(features.ids)
        passes, counts = [], None
        with native.Context(0) as ctx:
            for k in range(args.runs + 1):          # (pass 0 warms the device: dropped)
                native.prof_enable(True)
                total = np.zeros(n_genes + 3, np.int64)
                for chrom in chroms:
                    with ctx.begin_reads() as dr:
                        if not dr.add_bam(source, chrom):
                            continue
                        dr.finish()
                        dr.strand_tally(covers.get(chrom))
                        dr.gene_counts(n_genes, *maps.get(chrom, (None, None)), out=total)
                report = {r["kernel"]: r for r in native.prof_report() if r["kernel"] in KERNELS}
                if k:
                    passes.append({name: {"ms": r["ms"], "bytes": r["bytes"], "calls": r["calls"]} for name, r in report.items()})
                counts = total
    finally:
        source.close()
    print("RESULT " + json.dumps({"passes": passes, "counts": counts.tolist(), "map_entries": int(sum(m[0][0].shape[0] for m in maps.values())),
                                  "cover_entries": int(sum(c[0].shape[0] for c in covers.values()))}), flush=True)


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
    if args.child == "genecounts":
        argv = ["genecounts", "-B", args.prefix + ".bam", "-A", args.prefix + ".gtf", "-o", args.prefix + ".gc"]
    else:
        argv = ["strandedness", "-B", args.prefix + ".bam", "-A", args.prefix + ".gff", "-o", args.prefix + ".strand.txt"]
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
    last = [line for line in "".join(logged).splitlines() if ".genecounts.tsv: " in line]
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
    from spliser_amd import genecounts as gc, native, synth
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
        write_annotation(wl.genome, prefix + ".gtf", prefix + ".gff")
        say("%s (scale %g): %d reads, %d ops, %d chromosomes, %.1f MB BAM, %.1f MB GTF" % (name, scale, n_reads, n_ops, len(wl.genome.chrom_names), os.path.getsize(prefix + ".bam") / 1e6,
                                                                                         os.path.getsize(prefix + ".gtf") / 1e6))
        # (b) on the host, from the workload's own arrays: every read's result, the counts, the run heads
        t = time.perf_counter()
        features = gc.read_features(prefix + ".gtf")
        reader_s = time.perf_counter() - t
        n_genes = len(features.ids)
        maps = gc.maps_of(features, wl.genome.chrom_names)
        host_counts, heads, eligible_ops = np.zeros(n_genes + 3, np.int64), 0, 0
        for chrom, rs in zip(wl.genome.chrom_names, wl.reads):
            res = results_of(rs, maps.get(chrom, ((np.zeros(0, np.int32), np.zeros(0, np.uint32)), None))[0])
            host_counts += np.bincount(np.where(res >= 0, res, n_genes - 1 - res), minlength=n_genes + 3)
            heads += run_heads(res)
        del wl
        say("%s annotation: %d genes, %d map entries; read_features %.3f s" % (name, n_genes, sum(m[0][0].shape[0] for m in maps.values()), reader_s))
        res, why = run_child(args, "kernels", prefix)
        if res is None:
            say("%s kernels: FAILED: %s -- stopping" % (name, why))
            failed = True
            break
        same = res["counts"] == host_counts.tolist()
        say("%s counts: %d counted, %d no feature, %d ambiguous, %d not counted; the device's equal the host restatement's: %s" % (
            name, int(host_counts[:n_genes].sum()), int(host_counts[n_genes]), int(host_counts[n_genes + 1]), int(host_counts[n_genes + 2]), same))
        if not same:
            failed = True
            break
        ms = {k: statistics.median(p[k]["ms"] for p in res["passes"]) for k in KERNELS}
        say("%s (a) device events, ms summed over the chromosomes, median of %d passes: spl_gene_count %.3f ms, spl_strand_tally (cover map of %d entries) %.3f ms: %.2f x  %s" % (
            name, len(res["passes"]), ms[KERNELS[0]], res["cover_entries"], ms[KERNELS[1]], ms[KERNELS[0]] / ms[KERNELS[1]] if ms[KERNELS[1]] else 0.0,
            json.dumps([{k: round(p[k]["ms"], 3) for k in KERNELS} for p in res["passes"]])))
        counted = int(host_counts[:n_genes].sum())
        say("%s (b) global atomics: %d run heads for %d reads = %.4f a read (%.4f a counted read); a naive histogram issues one a counted read: %d" % (
            name, heads, n_reads, heads / float(n_reads), heads / float(max(counted, 1)), counted))
        floor_bytes = 10.0 * n_reads + 4.0 * n_ops
        say("%s (c) bytes floor: 10 B a read + 4 B an op = %.3f GB = %.3f ms at 8 TB/s; the kernel takes %.3f ms: %.1f %% of 8 TB/s, %.2f G reads/s" % (
            name, floor_bytes / 1e9, floor_bytes / HBM_BYTES_PER_S * 1e3, ms[KERNELS[0]], 100.0 * floor_bytes / HBM_BYTES_PER_S / (ms[KERNELS[0]] / 1e3), n_reads / (ms[KERNELS[0]] / 1e3) / 1e9))
        walls, readers, summary = {"genecounts": [], "strandedness": []}, [], ""
        for k in range(args.runs + 1):          # (round 0 warms the page cache and the device: dropped)
            for mode in ("genecounts", "strandedness"):
                r, why = run_child(args, mode, prefix)
                if r is None:
                    say("%s %s run %d: FAILED: %s -- stopping" % (name, mode, k, why))
                    failed = True
                    break
                if k:
                    walls[mode].append(r["wall_s"])
                    if mode == "genecounts":
                        readers.append(r["reader_s"])
                        summary = r["summary"]
            if failed:
                break
        if failed:
            break
        for mode in ("genecounts", "strandedness"):
            w = walls[mode]
            say("%s (d) `%s%s`: median %.4f s, min %.4f, max %.4f  %s" % (name, mode, " -A" if mode == "strandedness" else "", statistics.median(w), min(w), max(w), ["%.4f" % x for x in w]))
        say("%s (d) the annotation reader: median %.3f s = %.0f %% of the command" % (name, statistics.median(readers), 100.0 * statistics.median(readers) / statistics.median(walls["genecounts"])))
        say("    " + summary)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
