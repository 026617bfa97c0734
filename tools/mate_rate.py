#!/usr/bin/env python3
"""What `genecounts --fragments` costs: the decode with name keys beside the decode without, the three stages of the mate table,
the fragment kernel beside `spl_gene_count` on the same reads in the same run, the pairing's bytes floor, and the command beside
`genecounts` without the flag on the same file.
Runs on the GPU box; plain Python; every run is a fresh child under a time limit of its own, and the first failure ends everything.

    tools/mate_rate.py [--workloads arabidopsis,human] [--human-scale 0.25] [--runs 3] [--files DIR] [--out FILE]

Per workload (``synth.Workload``: the 20 M-read A. thaliana-shaped sample and the 50 M-read quarter of the human-shaped one that
tools/genecount_rate.py uses, the same seq-like BAM and GTF).  The workloads are single-end.  For the kernels they are made PAIRED
in memory: within a chromosome read i and read i + GAP (file order) become one fragment -- flags 99 / 147, one key for both, 64
mixed bits of (chromosome, i) given directly as the tests give theirs -- and go up with their keys (``upload_soa``), every read
pairable but those of a chromosome's last, incomplete stretch.  The FILE keeps the native writer's names, one per read: the
decode's cost does not depend on what the names say, and the command on it builds a mate table in which every read is alone (the
sort's and the searches' cost, not the second walk's).  Reported:
  (a) one child, the same file: `open_and_decode` with and without ``mate_keys``, alternating, wall clock to the end of the decode
      and the extraction kernels' device events (spl_prof_report), median of --runs passes;
  (b) one child, the paired arrays: per pass a fresh read set per chromosome, `spl_gene_count`, then `spl_gene_count_fragments`
      (which builds the table) under the library's stopwatch: compaction (mark, scan, scatter), the eight sort passes, the pair
      kernel, the fragment kernel, `spl_gene_count` -- device events, summed over the chromosomes, median of the passes;
  (c) the pairing's bytes floor -- 8 passes x 2 x 12 B per pairable read and 12 B per read -- and the share of 8 TB/s reached;
  (d) the command's wall clock with ``--fragments`` and without, a child each."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12
GAP = 37
STAGES = ("spl_mate_compact", "spl_mate_sort", "spl_mate_pair_kernel", "spl_gene_count_fragments_kernel", "spl_gene_count_kernel")
EXTRACT = ("spl_bam_extract_kernel",)


def paired(rs, k_chrom):
    """flags and keys that make read i and read i + GAP of every stretch of 2 GAP reads one fragment."""
    n = rs.n
    i = np.arange(n)
    whole = n - n % (2 * GAP)
    first = (i % (2 * GAP)) < GAP
    leader = np.where(first, i, i - GAP)
    flag = np.where(first, 99, 147).astype(np.uint16)
    flag[whole:] = 0          # (the last, incomplete stretch: single-end reads)
    h = (leader.astype(np.uint64) + np.uint64(1) + (np.uint64(k_chrom) << np.uint64(40))) * np.uint64(0x9E3779B97F4A7C15)          # (a bijection of 64 bits, then the finisher's two rounds)
    for mult in (0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53):
        h = (h ^ (h >> np.uint64(33))) * np.uint64(mult)
    keys = h ^ (h >> np.uint64(33))
    keys[keys < np.uint64(2)] = np.uint64(2)          # (never "no name")
    keys[whole:] = 0
    return flag, keys


def child_decode(args):
    sys.path.insert(0, HERE)
    import torch  # noqa: F401  (first: one HIP runtime per process)
    from spliser_amd import native, process
    quiet = lambda m: None
    out = {"plain": [], "keys": []}
    for k in range(2 * (args.runs + 1)):          # (the first of each warms the page cache and the device: dropped)
        which = "keys" if k % 2 else "plain"
        native.prof_enable(True)
        t = time.perf_counter()
        source = process.open_and_decode(args.prefix + ".bam", (0,), True, 16, process.DecodeOptions(mate_keys=which == "keys"), log=quiet)
        try:
            source.wait_all()
            assert source.join_decoders(), source.decline_reason()
            wall = time.perf_counter() - t
            ms = sum(r["ms"] for r in native.prof_report() if r["kernel"] in EXTRACT)
        finally:
            source.close()
        process.wait_deferred_close()
        if k >= 2:
            out[which].append({"wall_s": wall, "extract_ms": ms})
    print("RESULT " + json.dumps(out), flush=True)


def child_kernels(args):
    sys.path.insert(0, HERE)
    import torch  # noqa: F401
    from spliser_amd import genecounts as gc, native, synth
    wl = synth.Workload.load(args.cache_file, args.workload) if os.path.exists(args.cache_file) else synth.Workload(args.workload, scale=args.scale, workers=16)
    chroms = list(wl.genome.chrom_names)
    features = gc.read_features(args.prefix + ".gtf")
    maps = gc.maps_of(features, chroms)
    n_genes = len(features.ids)
    arrays, n_pairable = [], 0
    for k, rs in enumerate(wl.reads):
        flag, keys = paired(rs, k)
        arrays.append(native.ReadArrays(rs.pos, flag, rs.cig_off, rs.cigar, name_key=keys))
        n_pairable += int((flag != 0).sum())
    passes, stats, sums = [], None, None
    with native.Context(0) as ctx:
        with ctx.upload_soa(arrays, with_keys=True) as soa:
            for k in range(args.runs + 1):          # (pass 0 warms the device: dropped)
                native.prof_enable(True)
                reads, frags = np.zeros(n_genes + 3, np.int64), np.zeros(n_genes + 3, np.int64)
                stats = np.zeros(3, np.int64)
                for c, chrom in enumerate(chroms):
                    if not arrays[c].n:
                        continue
                    with ctx.begin_reads() as dr:
                        dr.add_soa(soa, c)
                        dr.finish()
                        a, b = maps.get(chrom, (None, None))
                        dr.gene_counts(n_genes, a, b, out=reads)
                        dr.gene_counts(n_genes, a, b, out=frags, fragments=True)
                        s = dr.mate_table(0)[1]
                        stats += [s["pairable"], s["paired"], s["unpaired_mate_mapped"]]
                report = {r["kernel"]: r for r in native.prof_report() if r["kernel"] in STAGES}
                if k:
                    passes.append({name: report[name]["ms"] if name in report else 0.0 for name in STAGES})
                sums = (int(reads.sum()), int(frags.sum()))
    print("RESULT " + json.dumps({"passes": passes, "stats": stats.tolist(), "sums": sums, "n_pairable": n_pairable, "n_reads": sum(a.n for a in arrays)}), flush=True)


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
    argv = ["genecounts", "-B", args.prefix + ".bam", "-A", args.prefix + ".gtf", "-o", args.prefix + "." + args.child] + (["--fragments"] if args.child == "fragments" else [])
    so = sys.stdout
    t = time.perf_counter()
    sys.stdout = Tee()
    try:
        assert cli.main(argv) == 0
    finally:
        sys.stdout = so
    wall = time.perf_counter() - t
    process.wait_deferred_close()
    last = [line for line in "".join(logged).splitlines() if ".genecounts.tsv: " in line or line.startswith("  mates: ")]
    print("RESULT " + json.dumps({"wall_s": wall, "summary": " | ".join(x.strip() for x in last)}), flush=True)


def run_child(args, mode, prefix, extra=()):
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--prefix", prefix, "--runs", str(args.runs)] + list(extra)
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
    ap.add_argument("--limit", type=int, default=400, help="seconds a child may take")
    ap.add_argument("--child", default=None)
    ap.add_argument("--prefix", default=None)
    ap.add_argument("--workload", default=None)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--cache-file", dest="cache_file", default=None)
    args = ap.parse_args()
    if args.child == "decode":
        return child_decode(args)
    if args.child == "kernels":
        return child_kernels(args)
    if args.child:
        return child_command(args)
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tools"))
    from spliser_amd import native, synth
    import genecount_rate
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
        if not os.path.exists(cache):
            wl.save(cache)
        n_reads, n_ops = sum(r.n for r in wl.reads), sum(int(r.cig_off[-1]) for r in wl.reads)
        if not os.path.exists(prefix + ".bam"):
            native.write_bam(prefix + ".bam", wl.genome.chrom_names, wl.genome.chrom_lengths, wl.reads, level=1, threads=16, seq_mode=1)
        genecount_rate.write_annotation(wl.genome, prefix + ".gtf", prefix + ".gff")
        del wl
        say("%s (scale %g): %d reads, %d ops, %.1f MB BAM" % (name, scale, n_reads, n_ops, os.path.getsize(prefix + ".bam") / 1e6))
        res, why = run_child(args, "decode", prefix)
        if res is None:
            say("%s decode: FAILED: %s -- stopping" % (name, why))
            failed = True
            break
        for which in ("plain", "keys"):
            w, e = [p["wall_s"] for p in res[which]], [p["extract_ms"] for p in res[which]]
            say("%s (a) decode %s: wall median %.4f s %s; extraction kernels %.3f ms %s" % (name, "with name keys" if which == "keys" else "without keys ", statistics.median(w),
                                                                                           ["%.4f" % x for x in w], statistics.median(e), ["%.3f" % x for x in e]))
        res, why = run_child(args, "kernels", prefix, ["--workload", name, "--scale", str(scale), "--cache-file", cache])
        if res is None:
            say("%s kernels: FAILED: %s -- stopping" % (name, why))
            failed = True
            break
        pairable, paired_reads, lonely = res["stats"]
        say("%s paired in memory (read i with read i + %d): %d reads, %d pairable, %d pairs, %d alone; rows sum to %d per read and %d per fragment (reads - pairs: %s)" % (
            name, GAP, res["n_reads"], pairable, paired_reads // 2, pairable - paired_reads, res["sums"][0], res["sums"][1], res["sums"][1] == res["n_reads"] - paired_reads // 2))
        if res["sums"][1] != res["n_reads"] - paired_reads // 2 or pairable != res["n_pairable"]:
            failed = True
            break
        ms = {k: statistics.median(p[k] for p in res["passes"]) for k in STAGES}
        say("%s (b) device events, ms summed over the chromosomes, median of %d passes: compaction %.3f, eight sort passes %.3f, pair kernel %.3f; fragment kernel %.3f beside spl_gene_count %.3f (%.2f x)  %s" % (
            name, len(res["passes"]), ms[STAGES[0]], ms[STAGES[1]], ms[STAGES[2]], ms[STAGES[3]], ms[STAGES[4]], ms[STAGES[3]] / ms[STAGES[4]] if ms[STAGES[4]] else 0.0,
            json.dumps([{k: round(v, 3) for k, v in p.items()} for p in res["passes"]])))
        floor_bytes = 8.0 * 2.0 * 12.0 * pairable + 12.0 * res["n_reads"]
        pairing_ms = ms[STAGES[0]] + ms[STAGES[1]] + ms[STAGES[2]]
        say("%s (c) pairing's bytes floor: 8 x 2 x 12 B a pairable read + 12 B a read = %.3f GB = %.3f ms at 8 TB/s; the three stages take %.3f ms: %.1f %% of 8 TB/s, %.2f G reads/s" % (
            name, floor_bytes / 1e9, floor_bytes / HBM_BYTES_PER_S * 1e3, pairing_ms, 100.0 * floor_bytes / HBM_BYTES_PER_S / (pairing_ms / 1e3) if pairing_ms else 0.0,
            res["n_reads"] / (pairing_ms / 1e3) / 1e9 if pairing_ms else 0.0))
        walls, summary = {"reads": [], "fragments": []}, {}
        for k in range(args.runs + 1):          # (round 0 warms the page cache and the device: dropped)
            for mode in ("reads", "fragments"):
                r, why = run_child(args, mode, prefix)
                if r is None:
                    say("%s genecounts (%s) run %d: FAILED: %s -- stopping" % (name, mode, k, why))
                    failed = True
                    break
                if k:
                    walls[mode].append(r["wall_s"])
                    summary[mode] = r["summary"]
            if failed:
                break
        if failed:
            break
        for mode in ("reads", "fragments"):
            w = walls[mode]
            say("%s (d) `genecounts%s`: median %.4f s, min %.4f, max %.4f  %s" % (name, " --fragments" if mode == "fragments" else "", statistics.median(w), min(w), max(w), ["%.4f" % x for x in w]))
            say("    " + summary[mode])
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
