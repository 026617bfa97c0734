#!/usr/bin/env python3
"""The genome on the device and the motif walk, measured (run on the GPU box).

    tools/genome_rate.py [--bases 3100000000] [--reads 20000000] [--dir DIR] [--device 0] [--passes 3] [--skip genome|motif] [--commands]

GENOME: a synthetic FASTA of human shape -- ``--bases`` bases in 25 sequences, 60-base lines, soft-masked stretches and runs of N --
is written to a temporary file (one 64 MiB block of lines repeated: the rate does not depend on the letters) and loaded with
``spl_genome_open`` ``--passes`` + 1 times, a fresh handle each.  Printed per pass: wall seconds, the device time of the copies and
of the kernels (``spl_genome_stats``), GB/s of text; beside them the link in the same session, twice: ``tools/pcie_rate.py``'s own
line (run as a child on the 20 M-read workload, whose cache under ``--cache`` is written if it is not there: the rate of a hand-over
through the staging ring, packing included) and the floor a plain copy sets (1 GiB from pinned memory in one copy, torch's
events); and the pack kernel's own time (``spl_prof_report``) as a fraction of 8 TB/s at its bytes floor,
1 B read and 0.5 B written a base.

MOTIF: the A. thaliana-shaped workload (``synth.Workload``) with ``--reads`` reads, every chromosome a fused set from ``upload_soa``
with zeroed strand bytes, a random genome of the workload's chromosome lengths on the device: ``spl_reads_motif_strand`` (the
library's stopwatch) beside ``spl_junctions`` mode 3 (``spl_junctions_stats``) on the same sets, device ms summed over the
chromosomes, the median of ``--passes`` passes.

COMMANDS (``--commands``): the same workload as a BAM whose records carry no aux fields (``native.write_bam``) and the random genome
as a FASTA of 60-base lines; ``junctions --genome g.fa --strandFromMotif`` beside ``junctions --strandFromXS`` and plain ``junctions``
on that one file, every run a fresh child under a time limit of its own, the three by turns, the first round dropped, wall seconds
of the child.  The XS run is a floor for that path: it walks the aux areas and finds no tag (a tagged twin of 20 M reads is not
written: the library's BAM writer writes no aux fields)."""
import argparse
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spliser_amd import native, synth  # noqa: E402

HBM_GBS = 8000.0


def write_fasta(path, lengths, line=60, seed=1):
    rng = np.random.default_rng(seed)
    rows = (64 << 20) // (line + 1)
    letters = np.frombuffer(b"ACGTACGTACGTACGTacgtN", np.uint8)
    block = np.empty((rows, line + 1), np.uint8)
    block[:, :line] = letters[rng.integers(0, len(letters), (rows, line))]
    block[:, line] = 10
    flat = block.reshape(-1).tobytes()
    with open(path, "wb") as fh:
        for k, n in enumerate(lengths):
            fh.write(b">chr%d synthetic\n" % (k + 1))
            full, rest = divmod(n, line)
            while full:
                take = min(full, rows)
                fh.write(flat[:take * (line + 1)])
                full -= take
            if rest:
                fh.write(flat[:rest] + b"\n")
    return os.path.getsize(path)


def link_floor(device):
    import torch
    host = torch.empty(1 << 30, dtype=torch.uint8).pin_memory()
    dev = torch.empty(1 << 30, dtype=torch.uint8, device="cuda:%d" % device)
    best = 0.0
    for _ in range(4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dev.copy_(host, non_blocking=True)
        b.record()
        b.synchronize()
        best = max(best, (1 << 30) / (a.elapsed_time(b) * 1e-3) / 1e9)
    del host, dev
    torch.cuda.empty_cache()
    return best


def pcie_rate_line(args, wl, say):
    """tools/pcie_rate.py in a child of its own, on the workload it reads from the cache: its last line."""
    cache = os.path.join(args.cache, "arabidopsis_s1_seed%d.npz" % synth.WORKLOADS["arabidopsis"]["seed"])
    if args.cache != "/tmp/wl":
        say("tools/pcie_rate.py: not run (it reads /tmp/wl)")
        return
    if not os.path.exists(cache):
        if wl is None or args.reads != synth.WORKLOADS["arabidopsis"]["n_reads"]:
            say("tools/pcie_rate.py: not run (its workload, %s, is not there and this run makes another)" % cache)
            return
        os.makedirs(args.cache, exist_ok=True)
        wl.save(cache)
    done = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "pcie_rate.py"), "3"],
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if done.returncode:
        raise RuntimeError("tools/pcie_rate.py ended with %d: %s" % (done.returncode, done.stderr[-2000:]))
    say("tools/pcie_rate.py, same session: " + done.stdout.strip().splitlines()[-1])


def genome_leg(args, say):
    share = np.array([8.0, 7.8, 6.4, 6.1, 5.8, 5.5, 5.1, 4.7, 4.5, 4.3, 4.4, 4.3, 3.7, 3.5, 3.3, 2.9, 2.7, 2.6, 1.9, 2.1, 1.5, 1.6, 5.0, 1.8, 0.5])
    lengths = (share / share.sum() * args.bases).astype(np.int64)
    path = os.path.join(args.dir, "genome_rate.fa")
    t = time.perf_counter()
    size = write_fasta(path, lengths.tolist())
    say("FASTA: %d bases in %d sequences, %.2f GB of text, written in %.1f s" % (int(lengths.sum()), len(lengths), size / 1e9, time.perf_counter() - t))
    floor = link_floor(args.device)
    say("link floor this session: %.1f GB/s (1 GiB, pinned, one copy) = %.3f s for the file" % (floor, size / floor / 1e9))
    try:
        with native.Context(args.device) as ctx:
            for k in range(args.passes + 1):
                native.prof_enable(True)
                t = time.perf_counter()
                g = native.Genome(ctx, path)
                wall = time.perf_counter() - t
                st = g.stats()
                pack = [r for r in native.prof_report() if r["kernel"] == "spl_genome_pack_kernel"]
                native.prof_enable(False)
                pack_ms = pack[0]["ms"] if pack else float("nan")
                say("pass %d%s: wall %.3f s = %.1f GB/s of text (%.2f x the floor's time); copies %.1f ms, kernels %.1f ms, of which the pack kernel %.2f ms = %.1f %% of 8 TB/s "
                    "at 1.5 B a base; %d sequences, %.2f GB on the device"
                    % (k, " (cold)" if k == 0 else "", wall, size / wall / 1e9, wall / (size / floor / 1e9), st["upload_ms"], st["pack_ms"], pack_ms,
                       100.0 * (1.5 * float(lengths.sum()) / (pack_ms * 1e-3) / 1e9) / HBM_GBS, len(g.names), st["device_bytes"] / 1e9))
                assert g.lengths == lengths.tolist()
                g.free()
    finally:
        os.remove(path)


def motif_leg(args, wl, say):
    names, lengths = wl.genome.chrom_names, wl.genome.chrom_lengths
    path = os.path.join(args.dir, "genome_rate_motif.fa")
    rng = np.random.default_rng(5)
    with open(path, "wb") as fh:
        for n, ln in zip(names, lengths):
            fh.write(b">" + n.encode() + b"\n")
            fh.write(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(ln))].tobytes() + b"\n")      # (one line a chromosome: the other leg measures the pack)
    try:
        with native.Context(args.device) as ctx, native.Genome(ctx, path) as g:
            sets = []
            for rs in wl.reads:
                arrays = native.ReadArrays(rs.pos, rs.flag, rs.cig_off, rs.cigar, xs=np.zeros(rs.n, np.uint8))
                soa = ctx.upload_soa([arrays], with_strand=True)
                dr = ctx.begin_reads(rs.n)
                dr.add_soa(soa, 0)
                sets.append((soa, dr.finish()))
            motif_ms, junction_ms, tally = [], [], None
            for k in range(args.passes + 1):
                native.prof_enable(True)
                tally = sum(dr.motif_strand(g, name) for (_, dr), name in zip(sets, names))
                ms = sum(r["ms"] for r in native.prof_report() if r["kernel"] == "spl_motif_strand_kernel")
                native.prof_enable(False)
                j = 0.0
                for _, dr in sets:
                    ctx.kernel_timing_begin(4)
                    dr.junctions(native.STRAND_FROM_XS, 8, 70, 500000)
                    j += dr.junctions_stats()[1]
                    ctx.kernel_timing_collect()
                if k:
                    motif_ms.append(ms)
                    junction_ms.append(j)
            n = sum(rs.n for rs in wl.reads)
            say("motif walk: %d reads, %d junction walks: spl_reads_motif_strand %.2f ms (passes %s), spl_junctions mode 3 on the same sets %.2f ms (passes %s)"
                % (n, int(tally[:7].sum()), statistics.median(motif_ms), ", ".join("%.2f" % v for v in motif_ms), statistics.median(junction_ms),
                   ", ".join("%.2f" % v for v in junction_ms)))
            say("  tally: " + ", ".join("%s %d" % kv for kv in zip(native.MOTIF_TALLY, tally.tolist())))
            for soa, dr in sets:
                dr.free()
                soa.free()
    finally:
        os.remove(path)


def commands_leg(args, wl, say):
    names, lengths = wl.genome.chrom_names, wl.genome.chrom_lengths
    bam, fa = os.path.join(args.dir, "genome_rate.bam"), os.path.join(args.dir, "genome_rate_cmd.fa")
    native.write_bam(bam, names, lengths, wl.reads, level=1, threads=16, seq_mode=1)
    rng = np.random.default_rng(5)
    with open(fa, "wb") as fh:
        for n, ln in zip(names, lengths):
            body = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(ln))]
            full = int(ln) // 60 * 60
            rows = np.empty((full // 60, 61), np.uint8)
            rows[:, :60] = body[:full].reshape(-1, 60)
            rows[:, 60] = 10
            fh.write(b">" + n.encode() + b"\n" + rows.tobytes() + (body[full:].tobytes() + b"\n" if full < int(ln) else b""))
    say("commands: %d reads, %.1f MB BAM without aux fields, %.1f MB FASTA" % (sum(r.n for r in wl.reads), os.path.getsize(bam) / 1e6, os.path.getsize(fa) / 1e6))
    modes = [("plain", []), ("--strandFromXS", ["--strandFromXS"]), ("--genome --strandFromMotif", ["--genome", fa, "--strandFromMotif"])]
    walls = {m: [] for m, _ in modes}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        for k in range(args.passes + 1):
            for mode, flags in modes:
                cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "spliser_amd", "junctions", "-B", bam, "-o", os.path.join(args.dir, "genome_rate.bed")] + flags
                t = time.perf_counter()
                done = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
                wall = time.perf_counter() - t
                if done.returncode:
                    raise RuntimeError("junctions %s ended with %d: %s" % (mode, done.returncode, done.stderr[-2000:]))
                if k:
                    walls[mode].append(wall)
                elif "strand from motif" in done.stdout:
                    say("  " + [line for line in done.stdout.splitlines() if "strand from motif" in line][0].strip())
        for mode, _ in modes:
            say("junctions %s: median %.3f s of the child (%s)" % (mode, statistics.median(walls[mode]), ", ".join("%.3f" % w for w in walls[mode])))
    finally:
        for path in (bam, fa, os.path.join(args.dir, "genome_rate.bed")):
            if os.path.exists(path):
                os.remove(path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=float, default=3.1e9)
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--cache", default="/tmp/wl", help="where tools/pcie_rate.py finds its workload")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--skip", choices=["genome", "motif"], default=None)
    ap.add_argument("--commands", action="store_true", help="also the command lines on a BAM of the workload")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.bases = int(args.bases)
    made_dir = args.dir is None
    args.dir = args.dir or tempfile.mkdtemp()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    wl = None
    if args.skip != "motif":        # (before the process touches the GPU: the workload is made by forked workers)
        t = time.perf_counter()
        wl = synth.Workload("arabidopsis", n_reads=args.reads)
        say("workload: arabidopsis shape, %d reads, made in %.1f s" % (sum(r.n for r in wl.reads), time.perf_counter() - t))
    try:
        if args.skip != "genome":
            pcie_rate_line(args, wl, say)      # (a child of its own, before this process opens the GPU)
            genome_leg(args, say)
        if wl is not None:
            motif_leg(args, wl, say)
            if args.commands:
                commands_leg(args, wl, say)
    finally:
        if made_dir:
            shutil.rmtree(args.dir, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
