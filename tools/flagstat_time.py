#!/usr/bin/env python3
"""What --flagstat costs, and that it costs nothing when it is not given: `process` without -b on the seq-like BAM bench.py's
human-shaped e2e leg writes, the parent commit's tree and this one side by side.  Runs on the GPU box; plain Python; every run is a
fresh child under a time limit of its own, the trees alternate, and the first failure ends everything.

    tools/flagstat_time.py [--parent TREE] [--workloads human] [--scale S] [--runs 5] [--files DIR] [--out FILE]

--parent TREE: a checkout of the parent commit, built (libspliser_hip.so in place).  Per workload, --runs times: parent (flag
off), this tree (flag off), this tree (flag on).  Reported: every wall clock of cli.main(), medians, the parent's min-max spread
and whether this tree's two medians lie within it around the parent's median (boxes and runs differ by more than most changes do,
DESIGN 7: the spread of THIS session is the margin), and the record scan's and the reduce kernel's time from the library's own
stopwatch (spl_prof_report), both settings.  The synthetic file's records are single-end and without mates: the counting does the
same work per record whatever its flags say."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(args):
    sys.path.insert(0, args.tree)
    import torch  # noqa: F401  (first: one HIP runtime per process)
    from spliser_amd import cli, native, process
    quiet, so = open(os.devnull, "w"), sys.stdout
    native.prof_enable(True)
    argv = ["process", "-B", args.prefix + ".bam", "-o", args.prefix + "." + args.child] + (["--flagstat"] if args.child == "on" else [])
    t = time.perf_counter()
    sys.stdout = quiet
    try:
        assert cli.main(argv) == 0
    finally:
        sys.stdout = so
    wall = time.perf_counter() - t
    process.wait_deferred_close()
    kernels = {k["kernel"]: round(k["ms"], 3) for k in native.prof_report() if "scan" in k["kernel"] or "flagstat" in k["kernel"] or "extract" in k["kernel"]}
    print("RESULT " + json.dumps({"wall_s": wall, "kernels_ms": kernels}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--workloads", default="human")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--files", default="/tmp/wl_files")
    ap.add_argument("--cache", default="/tmp/wl")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--child", default=None)
    ap.add_argument("--tree", default=HERE)
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
    steps = ([("parent", os.path.abspath(args.parent), "off")] if args.parent else []) + [("this", HERE, "off"), ("this", HERE, "on")]
    failed = False
    for name in args.workloads.split(","):
        cfg = synth.WORKLOADS[name]
        prefix = os.path.join(args.files, "%s_s%g_q1" % (name, args.scale))
        if not os.path.exists(prefix + ".bam"):
            cache = os.path.join(args.cache, "%s_s%g_seed%d.npz" % (name, args.scale, cfg["seed"]))
            wl = synth.Workload.load(cache, name) if os.path.exists(cache) else synth.Workload(name, scale=args.scale, workers=16)
            native.write_bam(prefix + ".bam", wl.genome.chrom_names, wl.genome.chrom_lengths, wl.reads, level=1, threads=16, seq_mode=1)
            say("%s: %d reads, %.1f MB BAM" % (name, sum(r.n for r in wl.reads), os.path.getsize(prefix + ".bam") / 1e6))
            del wl
        walls, kernels = {}, {}
        for k in range(args.runs + 1):          # (round 0 warms the page cache and the pool of each tree: dropped)
            for tree, path, mode in steps:
                cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--tree", path, "--prefix", prefix]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                if p.returncode != 0:
                    say("%s %s %s run %d: FAILED with status %d -- stopping\n%s" % (name, tree, mode, k, p.returncode, p.stderr[-2000:]))
                    failed = True
                    break
                res = json.loads([line[7:] for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1])
                if k:
                    walls.setdefault((tree, mode), []).append(res["wall_s"])
                    kernels.setdefault((tree, mode), []).append(res["kernels_ms"])
            if failed:
                break
        if failed:
            break
        for key, w in walls.items():
            say("%s %s flag %s: median %.4f s, min %.4f, max %.4f  %s" % (name, key[0], key[1], statistics.median(w), min(w), max(w), ["%.4f" % x for x in w]))
            names = sorted(kernels[key][-1])
            say("    kernels (ms, median of the runs): %s" % json.dumps({n: round(statistics.median(r.get(n, 0.0) for r in kernels[key]), 3) for n in names}))
        if ("parent", "off") in walls:
            pw = walls[("parent", "off")]
            pm, spread = statistics.median(pw), max(pw) - min(pw)
            for mode in ("off", "on"):
                tw = statistics.median(walls[("this", mode)])
                say("%s flag %s: this tree's median %.4f s against the parent's %.4f +- %.4f (its own min-max spread): %s" % (
                    name, mode, tw, pm, spread, "WITHIN" if abs(tw - pm) <= spread else "OUTSIDE"))
        on, off = statistics.median(walls[("this", "on")]), statistics.median(walls[("this", "off")])
        say("%s flag on: %+.4f s over this tree's flag-off median" % (name, on - off))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
