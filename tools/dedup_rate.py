#!/usr/bin/env python3
"""What duplicate marking costs: the stages of `spl_reads_duplicates` beside `spl_mate_table` on the same reads in the same run,
`spl_reads_dedup` beside `spl_reads_subsample` at 0.5, and the `duplicates` command beside `junctions` on the same file.
Runs on the GPU box; plain Python; every run is a fresh child under a time limit of its own, and the first failure ends everything.

    tools/dedup_rate.py [--workloads arabidopsis,human] [--human-scale 0.25] [--runs 3] [--share 0.2] [--files DIR] [--out FILE]
    tools/dedup_rate.py --tree OTHER_CHECKOUT [...]     spl_reads_subsample alone, this tree and the other alternating

Per workload (``synth.Workload``: the 20 M-read A. thaliana-shaped sample and the 50 M-read quarter of the human-shaped one that
tools/mate_rate.py uses).  The workloads are single-end; they are made PAIRED in memory as tools/mate_rate.py makes them (read i and
read i + GAP of a chromosome are one fragment, flags 99 / 147, one key for both), and a seeded ``--share`` of the fragments is
copied under new keys: both reads once more, the arrays sorted by POS again (stable).  Reported:
  (a) one child, the arrays up with their keys: per pass a fresh read set per chromosome; under the library's stopwatch the mate
      table's three stages, then the stages of the marks -- leaders and their scan, the signature kernel, the sort word by word
      (W2: 8 passes, W1: 5, W0: 5, the gathers between them included), the mark kernel, the groups' sizes --, the compaction by
      mark (count, write) and `spl_reads_subsample` at 0.5 (count, write): device events, summed over the chromosomes, median of
      --runs passes;
  (b) the marks' stages as a multiple of the mate table's, and the compaction's rate beside the subsampling's;
  (c) (arabidopsis) the `duplicates` command's wall clock beside `junctions` on the same file, a child each.
``--tree``: (a)'s `spl_reads_subsample` stages alone from this checkout and from the other (its library built), alternating, --runs
children each: whether the second instantiation of the tile bodies moved the first."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATE = ("spl_mate_compact", "spl_mate_sort", "spl_mate_pair_kernel")
DUP = ("spl_dup_lead", "spl_dup_signature_kernel", "spl_dup_sort_w2", "spl_dup_sort_w1", "spl_dup_sort_w0", "spl_dup_mark_kernel", "spl_dup_groups_kernel")
DEDUP = ("spl_dedup_count_kernel", "spl_dedup_write_kernel")
SUBSAMPLE = ("spl_subsample_count_kernel", "spl_subsample_write_kernel")
STAGES = MATE + DUP + DEDUP + SUBSAMPLE
HALF = 1 << 31


def with_copies(rs, flag, keys, share, rng, gap):
    """The paired arrays with ``share`` of the fragments once more under new keys -> (pos, flag, cig_off, cigar, keys), sorted by POS."""
    n = rs.n
    leaders = np.flatnonzero(flag == 99)
    chosen = leaders[rng.random(len(leaders)) < share]
    mates = chosen + gap          # (tools/mate_rate.py: read i and read i + GAP)
    extra = np.concatenate((chosen, mates))
    index = np.concatenate((np.arange(n), extra))
    new_keys = np.concatenate((keys, keys[np.concatenate((chosen, chosen))] ^ np.uint64(0x5DEECE66D1234567)))
    new_keys[n:][new_keys[n:] < np.uint64(2)] = np.uint64(2)
    order = np.argsort(rs.pos[index], kind="stable")
    index, new_keys = index[order], new_keys[order]
    n_ops = np.diff(rs.cig_off.astype(np.int64))
    counts = n_ops[index]
    ends = np.cumsum(counts)
    words = np.repeat(rs.cig_off[index].astype(np.int64) - (ends - counts), counts) + np.arange(int(ends[-1]) if len(ends) else 0)
    return rs.pos[index], flag[index], np.concatenate(([0], ends)).astype(np.uint32), rs.cigar[words], new_keys


def child_kernels(args):
    sys.path.insert(0, args.tree or HERE)
    sys.path.insert(1, os.path.join(HERE, "tools"))
    import torch  # noqa: F401  (first: one HIP runtime per process)
    from spliser_amd import native, synth
    import mate_rate
    wl = synth.Workload.load(args.cache_file, args.workload) if os.path.exists(args.cache_file) else synth.Workload(args.workload, scale=args.scale, workers=16)
    rng = np.random.default_rng(20261021)
    arrays = []
    for k, rs in enumerate(wl.reads):
        flag, keys = mate_rate.paired(rs, k)
        pos, flag, off, cigar, keys = with_copies(rs, flag, keys, args.share, rng, mate_rate.GAP)
        arrays.append(native.ReadArrays(pos, flag, off, cigar, name_key=keys))
    del wl
    only_subsample = args.child == "subsample"
    passes, counts, kept = [], None, None
    with native.Context(0) as ctx:
        with ctx.upload_soa(arrays, with_keys=True) as soa:
            for k in range(args.runs + 1):          # (pass 0 warms the device: dropped)
                native.prof_enable(True)
                counts, kept = np.zeros(7, np.int64), [0, 0]
                for c in range(len(arrays)):
                    if not arrays[c].n:
                        continue
                    with ctx.begin_reads() as dr:
                        dr.add_soa(soa, c)
                        dr.finish()
                        if not only_subsample:
                            dr.mate_table(0)
                            counts += [dr.duplicates(0)[1][name] for name in native.DUP_COUNTS]
                            left, n_left = dr.dedup()
                            left.free()
                            kept[0] += int(n_left.sum())
                        sel, n_sel = dr.subsample(0, HALF)
                        sel.free()
                        kept[1] += int(n_sel.sum())
                report = {r["kernel"]: r["ms"] for r in native.prof_report()}
                if k:
                    passes.append({name: report.get(name, 0.0) for name in STAGES})
    print("RESULT " + json.dumps({"passes": passes, "counts": None if counts is None else counts.tolist(), "kept": kept, "n_reads": sum(a.n for a in arrays)}), flush=True)


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
    argv = (["duplicates", "-B", args.prefix + ".bam", "-o", args.prefix + ".dups"] if args.child == "duplicates" else ["junctions", "-B", args.prefix + ".bam", "-o", args.prefix + ".rate.bed"])
    so = sys.stdout
    t = time.perf_counter()
    sys.stdout = Tee()
    try:
        assert cli.main(argv) == 0
    finally:
        sys.stdout = so
    wall = time.perf_counter() - t
    process.wait_deferred_close()
    last = [line for line in "".join(logged).splitlines() if line.startswith("Duplicates: ") or line.startswith("Junctions written")]
    print("RESULT " + json.dumps({"wall_s": wall, "summary": " | ".join(x.strip() for x in last)}), flush=True)


def run_child(args, mode, prefix, extra=()):
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--prefix", prefix, "--runs", str(args.runs), "--share", str(args.share)] + list(extra)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        return None, "status %d\n%s" % (p.returncode, p.stderr[-2000:])
    found = [line[7:] for line in p.stdout.splitlines() if line.startswith("RESULT ")]
    return (json.loads(found[-1]), "") if found else (None, "no RESULT line\n" + p.stdout[-2000:])


def median_of(passes, names):
    return statistics.median(sum(p[n] for n in names) for p in passes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="arabidopsis,human")
    ap.add_argument("--human-scale", type=float, default=0.25)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--share", type=float, default=0.2, help="the share of the fragments that is copied under new keys")
    ap.add_argument("--files", default="/tmp/wl_files")
    ap.add_argument("--cache", default="/tmp/wl")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tree", default=None, help="another checkout of this project, its library built: spl_reads_subsample there and here, alternating")
    ap.add_argument("--limit", type=int, default=400, help="seconds a child may take")
    ap.add_argument("--child", default=None)
    ap.add_argument("--prefix", default=None)
    ap.add_argument("--workload", default=None)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--cache-file", dest="cache_file", default=None)
    args = ap.parse_args()
    if args.child in ("kernels", "subsample"):
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
        if name == "arabidopsis" and not args.tree and not os.path.exists(prefix + ".bam"):
            native.write_bam(prefix + ".bam", wl.genome.chrom_names, wl.genome.chrom_lengths, wl.reads, level=1, threads=16, seq_mode=1)
        del wl
        common = ["--workload", name, "--scale", str(scale), "--cache-file", cache]
        if args.tree:
            got = {"here": [], "there": []}
            for k in range(args.runs):
                for which, tree in (("there", ["--tree", os.path.abspath(args.tree)]), ("here", [])):
                    res, why = run_child(args, "subsample", prefix, common + tree)
                    if res is None:
                        say("%s spl_reads_subsample (%s): FAILED: %s -- stopping" % (name, which, why))
                        return 1
                    got[which].append(median_of(res["passes"], SUBSAMPLE))
            for which in ("there", "here"):
                v = got[which]
                say("%s spl_reads_subsample at 0.5, count + write, device events, %s: median %.3f ms, min %.3f, max %.3f  %s" % (
                    name, "the other tree" if which == "there" else "this tree     ", statistics.median(v), min(v), max(v), ["%.3f" % x for x in v]))
            continue
        res, why = run_child(args, "kernels", prefix, common)
        if res is None:
            say("%s kernels: FAILED: %s -- stopping" % (name, why))
            failed = True
            break
        c = dict(zip(("reads", "examined", "pairs", "singles", "dup_pairs", "dup_singles", "flagged"), res["counts"]))
        say("%s paired in memory, %g of the fragments copied: %d reads, %d examined, %d pair and %d single fragments, %d duplicate pairs, %d duplicate singles; dedup keeps %d reads, "
            "the selection at 0.5 %d" % (name, args.share, res["n_reads"], c["examined"], c["pairs"], c["singles"], c["dup_pairs"], c["dup_singles"], res["kept"][0], res["kept"][1]))
        ms = {k: statistics.median(p[k] for p in res["passes"]) for k in STAGES}
        say("%s (a) device events, ms summed over the chromosomes, median of %d passes: %s  %s" % (
            name, len(res["passes"]), ", ".join("%s %.3f" % (k, ms[k]) for k in STAGES), json.dumps([{k: round(v, 3) for k, v in p.items()} for p in res["passes"]])))
        mate, dup, dedup, sub = (median_of(res["passes"], names) for names in (MATE, DUP, DEDUP, SUBSAMPLE))
        sort = median_of(res["passes"], DUP[2:5])
        say("%s (b) the marks %.3f ms = %.2f x the mate table's %.3f ms (its 8 sort passes %.3f ms; the marks' 18 passes and 3 gathers %.3f ms = %.2f x); "
            "the compaction by mark %.3f ms (%.2f G reads/s) beside the selection at 0.5 %.3f ms (%.2f G reads/s)" % (
                name, dup, dup / mate if mate else 0.0, mate, ms["spl_mate_sort"], sort, sort / ms["spl_mate_sort"] if ms["spl_mate_sort"] else 0.0, dedup,
                res["n_reads"] / (dedup / 1e3) / 1e9 if dedup else 0.0, sub, res["n_reads"] / (sub / 1e3) / 1e9 if sub else 0.0))
        if name != "arabidopsis":
            continue
        walls, summary = {"junctions": [], "duplicates": []}, {}
        for k in range(args.runs + 1):          # (round 0 warms the page cache and the device: dropped)
            for mode in ("junctions", "duplicates"):
                r, why = run_child(args, mode, prefix)
                if r is None:
                    say("%s `%s` run %d: FAILED: %s -- stopping" % (name, mode, k, why))
                    failed = True
                    break
                if k:
                    walls[mode].append(r["wall_s"])
                    summary[mode] = r["summary"]
            if failed:
                break
        if failed:
            break
        for mode in ("junctions", "duplicates"):
            w = walls[mode]
            say("%s (c) `%s`: median %.4f s, min %.4f, max %.4f  %s" % (name, mode, statistics.median(w), min(w), max(w), ["%.4f" % x for x in w]))
            say("    " + summary[mode])
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
