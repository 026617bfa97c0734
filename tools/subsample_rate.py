#!/usr/bin/env python3
"""What subsampling costs: `spl_reads_subsample` against its bytes floor and beside `spl_junctions` on the same reads in the same run,
a chain of descending selections against as many selections from the full set, and the `saturation` command beside `process`
without `-b` on the same file.
Runs on the GPU box; plain Python; every run is a fresh child under a time limit of its own, and the first failure ends everything.

    tools/subsample_rate.py [--workloads arabidopsis,human] [--human-scale 0.25] [--runs 3] [--steps 20] [--files DIR] [--out FILE]

Per workload (``synth.Workload``: the 20 M-read A. thaliana-shaped sample and the 50 M-read quarter of the human-shaped one that
tools/mate_rate.py uses, the same seq-like BAM).  For the kernels every read gets a key of its own, 64 mixed bits of (chromosome, i)
given directly as the tests give theirs, and goes up with it (``upload_soa``).  Reported:
  (a) one child, all chromosomes as one fused set: per pass a selection at the fractions 0.05, 0.5 and 0.95 under the library's
      stopwatch -- launch 1 (count), the scans of the tiles' totals, launch 3 (write): device events, median of --runs passes --
      against the bytes floor: 12 B a read read by launch 1 (the key and a CIGAR offset; POS and FLAG only without a name), then by
      launch 3 the same again, 18 B a kept read read and written (POS, FLAG, cig_off, the key) and 4 B a kept op read and written;
  (b) in the same passes `spl_junctions` on the full set, its device time beside the selection's;
  (c) --steps descending selections, each from the one before, against --steps selections from the full set: wall clock around the
      calls (each waits for the device), median of the passes;
  (d) the `saturation` command's wall clock, split into decode, selections, junction tables, site tables (host) and counting
      passes, beside `process` without `-b` on the same file, a child each."""
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
FRACTIONS = (0.05, 0.5, 0.95)
KERNELS = ("spl_subsample_count_kernel", "spl_subsample_write_kernel")


def keys_of(n, k_chrom):
    h = (np.arange(n, dtype=np.uint64) + np.uint64(1) + (np.uint64(k_chrom) << np.uint64(40))) * np.uint64(0x9E3779B97F4A7C15)          # (a bijection of 64 bits, then the finisher's two rounds)
    for mult in (0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53):
        h = (h ^ (h >> np.uint64(33))) * np.uint64(mult)
    keys = h ^ (h >> np.uint64(33))
    keys[keys < np.uint64(2)] = np.uint64(2)          # (never "no name")
    return keys


def child_kernels(args):
    sys.path.insert(0, HERE)
    import torch  # noqa: F401  (first: one HIP runtime per process)
    from spliser_amd import native, synth
    wl = synth.Workload.load(args.cache_file, args.workload) if os.path.exists(args.cache_file) else synth.Workload(args.workload, scale=args.scale, workers=16)
    arrays = [native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, name_key=keys_of(rs.n, k)) for k, rs in enumerate(wl.reads)]
    n_reads, n_ops = sum(a.n for a in arrays), sum(int(a.cig_off[-1]) for a in arrays)
    out = {"n_reads": n_reads, "n_ops": n_ops, "fractions": {}, "junctions_ms": [], "chain_s": [], "independent_s": []}
    thresholds = [(k << 32) // args.steps for k in range(args.steps, 0, -1)]
    with native.Context(0) as ctx:
        with ctx.upload_soa(arrays, with_keys=True) as soa:
            with ctx.begin_reads(n_reads) as dr:
                for c in range(len(arrays)):
                    dr.add_soa(soa, c)
                dr.finish()
                for k in range(args.runs + 1):          # (pass 0 warms the device: dropped)
                    for f in FRACTIONS:
                        native.prof_enable(True)
                        t = time.perf_counter()
                        sel, kept = dr.subsample(0, int(f * 4294967296.0))
                        wall = time.perf_counter() - t
                        report = {r["kernel"]: r["ms"] for r in native.prof_report()}
                        n_kept = sel.n
                        sel.free()
                        if k:
                            out["fractions"].setdefault(str(f), []).append({"count_ms": report.get(KERNELS[0], 0.0), "write_ms": report.get(KERNELS[1], 0.0), "wall_ms": wall * 1e3,
                                                                            "kept": n_kept})
                    native.prof_enable(False)
                    ctx.kernel_timing_begin(64)
                    dr.junctions(0, 8, 70, 500000)
                    ms = dr.junctions_stats()[1]
                    ctx.kernel_timing_collect()
                    if k:
                        out["junctions_ms"].append(ms)
                    t = time.perf_counter()
                    cur = dr
                    for th in thresholds:
                        nxt, _ = cur.subsample(0, th)
                        if cur is not dr:
                            cur.free()
                        cur = nxt
                    cur.free()
                    chain = time.perf_counter() - t
                    t = time.perf_counter()
                    for th in thresholds:
                        nxt, _ = dr.subsample(0, th)
                        nxt.free()
                    if k:
                        out["chain_s"].append(chain)
                        out["independent_s"].append(time.perf_counter() - t)
    print("RESULT " + json.dumps(out), flush=True)


def child_command(args):
    sys.path.insert(0, HERE)
    import torch  # noqa: F401
    from spliser_amd import process, saturation
    quiet = lambda m: None
    timings = {}
    t = time.perf_counter()
    if args.child == "saturation":
        saturation.saturation(args.prefix + ".bam", args.prefix + ".sat", steps=args.steps, log=quiet, threads=16, timings=timings)
    else:
        timings = process.process(args.prefix + ".bam", None, args.prefix + ".proc", log=quiet, threads=16)
    wall = time.perf_counter() - t
    process.wait_deferred_close()
    print("RESULT " + json.dumps({"wall_s": wall, "timings": {k: v for k, v in timings.items() if isinstance(v, float)}}), flush=True)


def run_child(args, mode, prefix, extra=()):
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--prefix", prefix, "--runs", str(args.runs), "--steps", str(args.steps)] + list(extra)
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--files", default="/tmp/wl_files")
    ap.add_argument("--cache", default="/tmp/wl")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=400, help="seconds a child may take")
    ap.add_argument("--no-command", dest="command", default=True, action="store_false", help="leave (d) out")
    ap.add_argument("--child", default=None)
    ap.add_argument("--prefix", default=None)
    ap.add_argument("--workload", default=None)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--cache-file", dest="cache_file", default=None)
    args = ap.parse_args()
    if args.child == "kernels":
        return child_kernels(args)
    if args.child:
        return child_command(args)
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
        scale = args.human_scale if name == "human" else 1.0
        prefix = os.path.join(args.files, "%s_s%g_q1" % (name, scale))
        cache = os.path.join(args.cache, "%s_s%g_seed%d.npz" % (name, scale, cfg["seed"]))
        wl = synth.Workload.load(cache, name) if os.path.exists(cache) else synth.Workload(name, scale=scale, workers=16)
        if not os.path.exists(cache):
            wl.save(cache)
        if args.command and not os.path.exists(prefix + ".bam"):
            native.write_bam(prefix + ".bam", wl.genome.chrom_names, wl.genome.chrom_lengths, wl.reads, level=1, threads=16, seq_mode=1)
        del wl
        res, why = run_child(args, "kernels", prefix, ["--workload", name, "--scale", str(scale), "--cache-file", cache])
        if res is None:
            say("%s kernels: FAILED: %s -- stopping" % (name, why))
            failed = True
            break
        n_reads, n_ops = res["n_reads"], res["n_ops"]
        say("%s (scale %g): %d reads, %d ops, one fused set, a key a read" % (name, scale, n_reads, n_ops))
        for f in FRACTIONS:
            p = res["fractions"][str(f)]
            kept = p[0]["kept"]
            count_ms, write_ms, wall_ms = (statistics.median(x[k] for x in p) for k in ("count_ms", "write_ms", "wall_ms"))
            floor = 12.0 * n_reads * 2 + 2.0 * 18.0 * kept + 2.0 * 4.0 * n_ops * kept / max(n_reads, 1)
            say("%s (a) fraction %g: %d kept; count %.3f ms, write %.3f ms (device events), the call %.3f ms (wall, scans and the host's wait between the launches included); floor %.3f GB = %.3f ms "
                "at 8 TB/s: the two launches reach %.1f %% of 8 TB/s, %.2f G reads/s  %s" % (
                    name, f, kept, count_ms, write_ms, wall_ms, floor / 1e9, floor / HBM_BYTES_PER_S * 1e3, 100.0 * floor / HBM_BYTES_PER_S / ((count_ms + write_ms) / 1e3) if count_ms + write_ms else 0.0,
                    n_reads / ((count_ms + write_ms) / 1e3) / 1e9 if count_ms + write_ms else 0.0, json.dumps([{k: round(v, 3) for k, v in x.items()} for x in p])))
        say("%s (b) spl_junctions on the same set in the same passes: %.3f ms (device events)  %s" % (name, statistics.median(res["junctions_ms"]), ["%.3f" % x for x in res["junctions_ms"]]))
        say("%s (c) %d descending selections, each from the one before: %.4f s; %d selections from the full set: %.4f s (wall, median of %d)  %s %s" % (
            name, args.steps, statistics.median(res["chain_s"]), args.steps, statistics.median(res["independent_s"]), len(res["chain_s"]), ["%.4f" % x for x in res["chain_s"]],
            ["%.4f" % x for x in res["independent_s"]]))
        if not args.command:
            continue
        for mode in ("process", "saturation"):
            walls, last = [], None
            for k in range(2):          # (round 0 warms the page cache and the device: dropped)
                r, why = run_child(args, mode, prefix)
                if r is None:
                    say("%s %s: FAILED: %s -- stopping" % (name, mode, why))
                    failed = True
                    break
                if k:
                    walls.append(r["wall_s"])
                    last = r["timings"]
            if failed:
                break
            say("%s (d) `%s`: %.4f s  %s" % (name, "process (no -b)" if mode == "process" else "saturation --steps %d" % args.steps, walls[0],
                                            json.dumps({k: round(v, 4) for k, v in last.items()})))
        if failed:
            break
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
