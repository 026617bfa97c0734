#!/usr/bin/env python3
"""What `coverage` costs: its three device stages against their bytes floor, and the command beside `process` on the same file.
Runs on the GPU box; plain Python; every run is a fresh child under a time limit of its own, and the first failure ends everything.

    tools/coverage_rate.py [--workloads human,arabidopsis] [--scale S] [--runs 3] [--files DIR] [--out FILE] [--no-rocprof]

Per workload (``synth.Workload``: bench.py's human-shaped and A. thaliana samples, written once as a seq-like BAM): a warm-up, then
--runs times `coverage` and `process` (without -b), each a child of its own.  Reported per command the wall clocks of cli.main() and
their median; for `coverage` the library's own stopwatch (device events: spl_prof_report) over mark -- the clearing of the
difference array and the mark launches --, compact -- count, the scan of the tile counts, emit -- and scan -- the deltas' prefix
sums --, summed over the chromosomes, median of the runs; the mark stage's events a second (two a block: what the totals' runs and
reads say is a lower bound, the blocks themselves are not counted -- the figure uses reads that contributed, two events each, as the
floor of it); the bytes floor (4 bytes a position cleared and read, 10 bytes a read and 4 an op) and the share of 8 TB/s the three
stages together reach.  One more `coverage` child under ``rocprofv3 --kernel-trace --stats`` (the program behind ``--``) gives the
kernels' own times; its csv is summarised for the spl_cov_* and spl_sort_part_* kernels."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12
STAGES = ("spl_cov_mark_kernel", "spl_cov_compact", "spl_cov_scan")


def child(args):
    sys.path.insert(0, HERE)
    import torch  # noqa: F401  (first: one HIP runtime per process)
    from spliser_amd import cli, native, process
    logged = []

    class Tee(object):
        def write(self, text):
            logged.append(text)

        def flush(self):
            pass
    native.prof_enable(True)
    if args.child == "coverage":
        argv = ["coverage", "-B", args.prefix + ".bam", "-o", args.prefix + ".cov"]
    else:
        argv = ["process", "-B", args.prefix + ".bam", "-o", args.prefix + ".proc"]
    so = sys.stdout
    t = time.perf_counter()
    sys.stdout = Tee()
    try:
        assert cli.main(argv) == 0
    finally:
        sys.stdout = so
    wall = time.perf_counter() - t
    process.wait_deferred_close()
    report = native.prof_report()
    stages = {k["kernel"]: {"ms": round(k["ms"], 4), "bytes": k["bytes"], "calls": k["calls"]} for k in report if k["kernel"] in STAGES}
    decode_ms = round(sum(k["ms"] for k in report if k["kernel"] not in STAGES), 3)
    totals = [line for line in "".join(logged).splitlines() if line.endswith("contributed") or " contributed, " in line]
    print("RESULT " + json.dumps({"wall_s": wall, "stages": stages, "other_kernels_ms": decode_ms, "totals": totals}), flush=True)


def run_child(args, mode, prefix, wrap=()):
    cmd = ["timeout", "-k", "10", str(args.limit)] + list(wrap) + [sys.executable, os.path.abspath(__file__), "--child", mode, "--prefix", prefix]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        return None, "status %d\n%s" % (p.returncode, p.stderr[-2000:])
    found = [line[7:] for line in p.stdout.splitlines() if line.startswith("RESULT ")]
    return (json.loads(found[-1]), "") if found else (None, "no RESULT line\n" + p.stdout[-2000:])


def rocprof_summary(directory):
    """-> {kernel: (calls, total ms)} of the coverage kernels and the scans in a rocprofv3 --stats directory."""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name", "")
                if "spl_cov_" in name or "spl_sort_part_" in name or "spl_sort_digit_scan" in name:
                    short = re.search(r"spl_\w+", name).group(0)      # (the kernels live in an unnamed namespace: the name has brackets in front)
                    calls, ns = out.get(short, (0, 0.0))
                    out[short] = (calls + int(row.get("Calls", 0)), ns + float(row.get("TotalDurationNs", 0.0)))
    return {k: (c, ns / 1e6) for k, (c, ns) in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="human,arabidopsis")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--files", default="/tmp/wl_files")
    ap.add_argument("--cache", default="/tmp/wl")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--prefix", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    sys.path.insert(0, HERE)
    from spliser_amd import native, synth
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    os.makedirs(args.files, exist_ok=True)
    os.makedirs(args.cache, exist_ok=True)
    failed = False
    for name in args.workloads.split(","):
        cfg = synth.WORKLOADS[name]
        prefix = os.path.join(args.files, "%s_s%g_q1" % (name, args.scale))
        cache = os.path.join(args.cache, "%s_s%g_seed%d.npz" % (name, args.scale, cfg["seed"]))
        wl = synth.Workload.load(cache, name) if os.path.exists(cache) else synth.Workload(name, scale=args.scale, workers=16)
        n_reads, n_ops = sum(r.n for r in wl.reads), sum(int(r.cig_off[-1]) for r in wl.reads)
        length = sum(int(v) for v in wl.genome.chrom_lengths)
        if not os.path.exists(prefix + ".bam"):
            native.write_bam(prefix + ".bam", wl.genome.chrom_names, wl.genome.chrom_lengths, wl.reads, level=1, threads=16, seq_mode=1)
        say("%s (scale %g): %d reads, %d ops, %d chromosomes of %d bases in all, %.1f MB BAM" % (name, args.scale, n_reads, n_ops, len(wl.genome.chrom_names), length,
                                                                                              os.path.getsize(prefix + ".bam") / 1e6))
        del wl
        walls, stages, last = {"coverage": [], "process": []}, [], None
        for k in range(args.runs + 1):          # (round 0 warms the page cache and the device: dropped)
            for mode in ("coverage", "process"):
                res, why = run_child(args, mode, prefix)
                if res is None:
                    say("%s %s run %d: FAILED: %s -- stopping" % (name, mode, k, why))
                    failed = True
                    break
                if k:
                    walls[mode].append(res["wall_s"])
                    if mode == "coverage":
                        stages.append(res["stages"])
                        last = res
            if failed:
                break
        if failed:
            break
        for mode in ("coverage", "process"):
            w = walls[mode]
            say("%s `%s`: median %.4f s, min %.4f, max %.4f  %s" % (name, mode, statistics.median(w), min(w), max(w), ["%.4f" % x for x in w]))
        for line in last["totals"]:
            say("    " + line.strip())
        ms = {s: statistics.median(r.get(s, {"ms": 0.0})["ms"] for r in stages) for s in STAGES}
        calls = {s: stages[-1].get(s, {"calls": 0})["calls"] for s in STAGES}
        say("%s stages (device events, ms summed over the chromosomes, median of the runs): %s; calls %s" % (name, json.dumps({s: round(v, 3) for s, v in ms.items()}), json.dumps(calls)))
        say("%s other kernels of the command (the decode): %.1f ms" % (name, last["other_kernels_ms"]))
        floor_bytes = 2.0 * 4.0 * length + 10.0 * n_reads + 4.0 * n_ops
        all_ms = sum(ms.values())
        say("%s bytes floor: 4 B a position cleared and read + 10 B a read + 4 B an op = %.3f GB = %.3f ms at 8 TB/s; the three stages take %.3f ms: %.1f %% of 8 TB/s"
            % (name, floor_bytes / 1e9, floor_bytes / HBM_BYTES_PER_S * 1e3, all_ms, 100.0 * floor_bytes / HBM_BYTES_PER_S / (all_ms / 1e3) if all_ms else 0.0))
        contributed = 0
        for line in last["totals"]:
            words = line.replace(",", "").split()
            if "of" in words:
                contributed += int(words[words.index("of") - 1])
        if ms[STAGES[0]]:
            say("%s mark: at least %d events (two a contributing read) in %.3f ms, clearing included: %.2f G events/s at least" % (name, 2 * contributed, ms[STAGES[0]],
                                                                                                                          2 * contributed / (ms[STAGES[0]] / 1e3) / 1e9))
        if not args.no_rocprof:
            d = os.path.join(args.files, "rocprof_cov_%s" % name)
            res, why = run_child(args, "coverage", prefix, wrap=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"))
            if res is None:
                say("%s rocprofv3 run: FAILED: %s -- stopping" % (name, why))
                failed = True
                break
            for kernel, (n, total) in sorted(rocprof_summary(d).items(), key=lambda kv: -kv[1][1]):
                say("    rocprofv3 %-32s %6d calls %10.3f ms" % (kernel, n, total))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
