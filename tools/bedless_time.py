#!/usr/bin/env python3
"""What `process` without -b costs against `junctions` + `process -b`, on the files bench.py --full generates (seq-like BAMs).
Runs on the GPU box; plain Python; every GPU step is a fresh child under a time limit of its own, and the first failure ends the run.

    tools/bedless_time.py [--parent TREE] [--workloads human,arabidopsis] [--scale S] [--runs N] [--files DIR] [--out FILE]

--parent TREE: a checkout of the parent commit, built (libspliser_hip.so in place): its steps alternate with this tree's.
Without it only this tree is measured.  Per workload:
  1. wall clock of `process` without -b (this tree) and of `junctions` + `process -b` (both trees): median of --runs warm runs;
     SPL_PROCESS_TIMING's last line of each run is kept in the output
  2. `spl_junctions` on the largest chromosome's fused read set after a device decode: wall clock around the call (both trees:
     the parent's includes its layout launch) and, in this tree, the device time between HIP events (spl_junctions_stats)
  3. the lowest free device memory (hipMemGetInfo, polled every 2 ms) during the `junctions` command, both trees
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(args):
    """One step in one tree (sys.path[0] = that tree)."""
    sys.path.insert(0, args.tree)
    import torch  # noqa: F401  (first: one HIP runtime per process)
    from spliser_amd import cli, native, process
    prefix, mode = args.prefix, args.child
    quiet = open(os.devnull, "w")
    out = {"mode": mode, "tree": args.tree}

    def run_cli(argv):
        so, sys.stdout = sys.stdout, quiet
        try:
            assert cli.main(argv) == 0
        finally:
            sys.stdout = so
        process.wait_deferred_close()

    if mode in ("one", "two"):
        walls = []
        for k in range(args.runs + 1):      # (the first run is the cold one: dropped)
            t = time.perf_counter()
            if mode == "one":
                run_cli(["process", "-B", prefix + ".bam", "-o", prefix + ".one"])
            else:
                run_cli(["junctions", "-B", prefix + ".bam", "-o", prefix + ".j.bed"])
                t_mid = time.perf_counter()
                run_cli(["process", "-B", prefix + ".bam", "-b", prefix + ".j.bed", "-o", prefix + ".two"])
                out.setdefault("junctions_s", []).append(t_mid - t)
            if k:
                walls.append(time.perf_counter() - t)
        out["wall_s"] = walls
        out["median_s"] = statistics.median(walls)
    elif mode == "kernel":
        with native.Context(0) as ctx:
            bam = native.BamFile(prefix + ".bam", defer=True)
            try:
                assert bam.decode_on_device(ctx), bam.decline_reason()
                chrom = max(bam.ref_names, key=lambda c: bam.wait_ref(c)[0])
                walls, ms = [], []
                for k in range(args.runs + 1):
                    with ctx.begin_reads() as dr:
                        n = dr.add_bam(bam, chrom)
                        dr.finish()
                        ctx.sync()
                        if hasattr(dr, "junctions_stats"):
                            ctx.kernel_timing_begin(4)
                        t = time.perf_counter()
                        table = dr.junctions(0, 8, 70, 500000)
                        w = time.perf_counter() - t
                        if hasattr(dr, "junctions_stats"):
                            out["table_bytes"], m = dr.junctions_stats()
                            ctx.kernel_timing_collect()
                            ms.append(m)
                        out["record_bytes_after"] = dr.layout_bytes()[1]
                        if k:
                            walls.append(w)
                out.update(chrom=chrom, reads=n, junctions=len(table["left"]), wall_s=walls, median_wall_s=statistics.median(walls),
                           device_ms=ms[1:] if ms else None)
            finally:
                bam.close()
    elif mode == "mem":
        low = [None]
        stop = threading.Event()

        def poll():
            while not stop.is_set():
                free, _total = torch.cuda.mem_get_info(0)
                low[0] = free if low[0] is None else min(low[0], free)
                time.sleep(0.002)
        free0, total = torch.cuda.mem_get_info(0)
        th = threading.Thread(target=poll)
        th.start()
        try:
            run_cli(["junctions", "-B", prefix + ".bam", "-o", prefix + ".j.bed"])
        finally:
            stop.set()
            th.join()
        out.update(free_before=free0, lowest_free=low[0], peak_used_bytes=free0 - low[0])
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--workloads", default="human,arabidopsis")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--files", default="/tmp/wl_files")
    ap.add_argument("--cache", default="/tmp/wl")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=420, help="seconds a child may take")
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
    trees = [("this", HERE)] + ([("parent", os.path.abspath(args.parent))] if args.parent else [])
    for name in args.workloads.split(","):
        cfg = synth.WORKLOADS[name]
        prefix = os.path.join(args.files, "%s_s%g_q1" % (name, args.scale))
        if not os.path.exists(prefix + ".bam"):
            cache = os.path.join(args.cache, "%s_s%g_seed%d.npz" % (name, args.scale, cfg["seed"]))
            print("%s: making the files ..." % name, flush=True)
            if os.path.exists(cache):
                wl = synth.Workload.load(cache, name)
            else:
                wl = synth.Workload(name, scale=args.scale, workers=16)
                wl.save(cache)
            native.write_bam(prefix + ".bam", wl.genome.chrom_names, wl.genome.chrom_lengths, wl.reads, level=1, threads=16, seq_mode=1)
            say("%s: %d reads, %.1f MB BAM" % (name, sum(r.n for r in wl.reads), os.path.getsize(prefix + ".bam") / 1e6))
            del wl
        steps = [("one", "this")] + [(m, t) for m in ("two", "kernel", "mem") for t, _ in trees]
        for mode, tree in steps:
            path = dict(trees)[tree]
            # (this file runs the step in either tree: the parent has no such tool; the child puts the tree first on sys.path)
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--tree", path, "--prefix", prefix,
                   "--runs", str(args.runs)]
            env = dict(os.environ, SPL_PROCESS_TIMING="1")
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, text=True)
            if p.returncode != 0:
                say("%s %s %s: FAILED with status %d -- stopping\n%s" % (name, tree, mode, p.returncode, p.stderr[-2000:]))
                break
            res = [line[7:] for line in p.stdout.splitlines() if line.startswith("RESULT ")]
            say("%s %s %s: %s" % (name, tree, mode, res[-1] if res else "no result"))
            timing = [line for line in p.stderr.splitlines() if line.startswith("[process] open_s") or "junctions_s" in line]
            for line in timing[-2:]:
                say("    " + line)
        else:
            continue
        break
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
