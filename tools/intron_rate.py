#!/usr/bin/env python3
"""What `intronretention` costs: its kernel beside the three coverage stages that run in front of it in the same call (those stages
are the yardstick: this work leaves them as they were), its bytes floor, and the command beside `coverage` on the same file.
Runs on the GPU box; plain Python; every run is a fresh child under a time limit of its own, and the first failure ends everything.

    tools/intron_rate.py [--workloads arabidopsis,human] [--human-scale 0.25] [--runs 3] [--files DIR] [--out FILE]

Per workload: the two files of tools/genecount_rate.py with the same synthetic annotation (its ``write_annotation``).  Reported:
  (a) one child decodes the file on the device and runs, per chromosome on the same fused set, `spl_intron_depth` over the
      annotation's introns -- a warm-up pass, then --runs passes under the library's own stopwatch (device events around the
      launches: spl_prof_report), summed over the chromosomes, median of the passes and their spread: the mark, compact and scan
      stages and the intron kernel;
  (b) the introns: how many, their measurable bases, how many are long ones (a team each), how many have no measurable base;
  (c) the kernel's bytes floor (44 B an intron, 8 B a piece, 8 B a boundary -- every boundary read once, as if no two introns
      shared one and no pass were repeated) and the share of 8 TB/s the kernel reaches;
  (d) the command's wall clock beside `coverage`, a child each."""
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

STAGES = ("spl_cov_mark_kernel", "spl_cov_compact", "spl_cov_scan", "spl_intron_kernel")


def child_kernels(args):
    sys.path.insert(0, HERE)
    import torch  # noqa: F401  (first: one HIP runtime per process)
    from spliser_amd import genecounts as gc, intronretention as ir, native, process
    quiet = lambda m: None
    source = process.open_and_decode(args.prefix + ".bam", (0,), True, 16, process.DecodeOptions(), log=quiet)
    try:
        source.wait_all()
        assert source.join_decoders(), source.decline_reason()
        chroms = list(source.ref_names)
        lengths = dict(zip(source.ref_names, source.ref_lengths))
        table = ir.Table(gc.read_features(args.prefix + ".gtf"))
        pieces = {c: table.pieces(table.rows_on(c, "."), c, ".", lengths[c]) for c in chroms}
        passes, sums = [], None
        with native.Context(0) as ctx:
            for k in range(args.runs + 1):          # (pass 0 warms the device: dropped)
                native.prof_enable(True)
                sums = np.zeros(4, np.int64)
                for chrom in chroms:
                    with ctx.begin_reads() as dr:
                        if not dr.add_bam(source, chrom):
                            continue
                        dr.finish()
                        sums += dr.intron_depth(lengths[chrom], *pieces[chrom], trim_percent=30).sum(axis=0)
                report = {r["kernel"]: r for r in native.prof_report() if r["kernel"] in STAGES}
                if k:
                    passes.append({name: {"ms": r["ms"], "bytes": r["bytes"], "calls": r["calls"]} for name, r in report.items()})
    finally:
        source.close()
    n_pieces = sum(int(p[1].shape[0]) for p in pieces.values())
    print("RESULT " + json.dumps({"passes": passes, "sums": sums.tolist(), "n_pieces": n_pieces}), flush=True)


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
    argv = [args.child, "-B", args.prefix + ".bam", "-o", args.prefix + ".rate"] + (["-A", args.prefix + ".gtf"] if args.child == "intronretention" else [])
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
    last = [line for line in "".join(logged).splitlines() if ".introns.tsv: " in line or ".bedgraph: " in line]
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
    from spliser_amd import genecounts as gc, intronretention as ir, native, synth
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
        lengths = dict(zip(wl.genome.chrom_names, (int(v) for v in wl.genome.chrom_lengths)))
        del wl
        say("%s (scale %g): %d reads, %d ops, %d chromosomes, %.1f MB BAM, %.1f MB GTF" % (name, scale, n_reads, n_ops, len(lengths), os.path.getsize(prefix + ".bam") / 1e6,
                                                                                         os.path.getsize(prefix + ".gtf") / 1e6))
        # (b) the introns, on the host
        t = time.perf_counter()
        table = ir.Table(gc.read_features(prefix + ".gtf"))
        n_pieces, bases, n_long, n_none = 0, 0, 0, 0
        for chrom in table.chroms:
            off, start, end = table.pieces(table.rows_on(chrom, "."), chrom, ".", lengths.get(chrom))
            per = ir.no_read_numbers(off, start, end, 0)[:, 0]
            n_pieces, bases, n_long, n_none = n_pieces + int(start.shape[0]), bases + int(per.sum()), n_long + int((per >= native.INTRON_LONG_BASES).sum()), n_none + int((per == 0).sum())
        n_introns = int(table.gene.shape[0])
        say("%s (b) introns: %d of %d genes in %d pieces, %d measurable bases; %d long ones (>= %d bases: a team each), %d without a measurable base; tables made in %.3f s" % (
            name, n_introns, len(table.ids), n_pieces, bases, n_long, native.INTRON_LONG_BASES, n_none, time.perf_counter() - t))
        res, why = run_child(args, "kernels", prefix)
        if res is None:
            say("%s kernels: FAILED: %s -- stopping" % (name, why))
            failed = True
            break
        same = res["sums"][0] == bases and res["n_pieces"] == n_pieces
        say("%s sums over the introns: measurable %d, covered %d, depth_n %d, depth_sum %d; the device's measurable bases equal the host's: %s" % ((name,) + tuple(res["sums"]) + (same,)))
        if not same:
            failed = True
            break
        ms = {k: statistics.median(p[k]["ms"] for p in res["passes"] if k in p) if any(k in p for p in res["passes"]) else 0.0 for k in STAGES}
        say("%s (a) device events, ms summed over the chromosomes, median of %d passes: mark %.3f, compact %.3f, scan %.3f, intron kernel %.3f ms (%.2f x mark)  %s" % (
            name, len(res["passes"]), ms[STAGES[0]], ms[STAGES[1]], ms[STAGES[2]], ms[STAGES[3]], ms[STAGES[3]] / ms[STAGES[0]] if ms[STAGES[0]] else 0.0,
            json.dumps([{k: round(p[k]["ms"], 3) for k in STAGES if k in p} for p in res["passes"]])))
        floor_bytes = float(res["passes"][0][STAGES[3]]["bytes"])
        say("%s (c) bytes floor: 44 B an intron + 8 B a piece + 8 B a boundary = %.4f GB = %.4f ms at 8 TB/s; the kernel takes %.3f ms: %.2f %% of 8 TB/s, %.2f M introns/s" % (
            name, floor_bytes / 1e9, floor_bytes / gr.HBM_BYTES_PER_S * 1e3, ms[STAGES[3]], 100.0 * floor_bytes / gr.HBM_BYTES_PER_S / (ms[STAGES[3]] / 1e3) if ms[STAGES[3]] else 0.0,
            n_introns / (ms[STAGES[3]] / 1e3) / 1e6 if ms[STAGES[3]] else 0.0))
        walls, summary = {"intronretention": [], "coverage": []}, ""
        for k in range(args.runs + 1):          # (round 0 warms the page cache and the device: dropped)
            for mode in ("intronretention", "coverage"):
                r, why = run_child(args, mode, prefix)
                if r is None:
                    say("%s %s run %d: FAILED: %s -- stopping" % (name, mode, k, why))
                    failed = True
                    break
                if k:
                    walls[mode].append(r["wall_s"])
                    if mode == "intronretention":
                        summary = r["summary"]
            if failed:
                break
        if failed:
            break
        for mode in ("intronretention", "coverage"):
            w = walls[mode]
            say("%s (d) `%s`: median %.4f s, min %.4f, max %.4f  %s" % (name, mode, statistics.median(w), min(w), max(w), ["%.4f" % x for x in w]))
        say("    " + summary)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
