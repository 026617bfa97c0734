#!/usr/bin/env python3
"""SAM text parsed on the GPU against the link's floor and against the BAM decode of the same reads.

    tools/sam_decode_rate.py [--reads 2000000,20000000] [--dir DIR] [--device 0] [--out profiles/r12_sam_decode.txt]

Per size: a synthetic A. thaliana-shaped sample (``synth.Workload``) is written as SAM the way an aligner writes it -- read names,
pseudo-random SEQ and QUAL of the read's length, an ``NH:i`` / ``XS:A`` tail (``samio.write_sam``'s ``*`` columns would flatter the
rate: 60 bytes a read instead of ~300) -- and as a ``seq-like`` BAM.  Printed: seconds from ``spl_bam_decode_device`` until every
reference is complete (best of three after a warm-up, a fresh object each), GB/s of text beside the link's floor (text bytes at
the project's PCIe figure, 56 GB/s), the same call on the BAM, and for files of at most 2 M reads the Python reader's seconds for
the same file (``samio.read_sam``: what `-B x.sam` ran before this decoder).  The files are written once and removed at the end.

The same text is also written COMPRESSED, the way it lies on disk: as BGZF at level 6 with payloads of 0xff00 bytes (``bgzip``,
``samtools view -O sam,level=6``) and as gzip (members of 256 MiB of text, level 6, deflated side by side: the host's inflate reads
them as one stream).  Per form: seconds and GB/s of INFLATED text, against the plain text's figure of the same run and the BAM's;
for the BGZF leg one more call under ``SPL_BAM_TIMING`` gives the decoder's own split -- upload, inflate, parse."""
import argparse
import multiprocessing
import os
import sys
import tempfile
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spliser_amd import native, samio, synth  # noqa: E402

LINK_GBS = 56.0


def write_sam_like_an_aligner(path, names, lengths, read_sets, seed=1, piece=1_000_000):
    """-> lines written.  Columns built with numpy's string routines, a million reads at a time."""
    rng = np.random.default_rng(seed)
    bases, quals = np.frombuffer(b"ACGT", np.uint8), np.frombuffer(b"#,:AFJ", np.uint8)
    n_lines = 0
    with open(path, "wb") as fh:
        fh.write(b"@HD\tVN:1.6\tSO:coordinate\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n.encode("ascii"), ln) for n, ln in zip(names, lengths)))
        fh.write(b"@PG\tID:synth\tPN:sam_decode_rate\n")
        for name, rs in zip(names, read_sets):
            off = rs.cig_off.astype(np.int64)
            for lo in range(0, rs.n, piece):
                hi = min(rs.n, lo + piece)
                ops = rs.cigar[off[lo]:off[hi]]
                text = np.char.add((ops >> 4).astype("U"), np.array(list(samio.OP_CODES))[ops & 15]).astype(object)
                starts = off[lo:hi] - off[lo]
                cigar = np.add.reduceat(text, starts) if len(text) else np.array([], object)
                n_ops = np.diff(off[lo:hi + 1])
                code, length = ops & 15, (ops >> 4).astype(np.int64)
                qlen = np.add.reduceat(np.where(np.isin(code, (0, 1, 4, 7, 8)), length, 0), starts)
                spliced = np.add.reduceat((code == 3).astype(np.int64), starts) > 0
                L = int(qlen.max())
                seq = bases[rng.integers(0, 4, (hi - lo, L))]
                qual = quals[rng.integers(0, 6, (hi - lo, L))]
                flag = rs.flag[lo:hi].astype(np.int64)
                tail = np.where(spliced, np.where(flag & 16, "\tXS:A:-", "\tXS:A:+"), "")
                lines = []
                for k in range(hi - lo):
                    q = int(qlen[k])
                    c = cigar[k] if n_ops[k] else "*"
                    lines.append(b"read.%d\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\tNH:i:1%s\n" % (n_lines + k, flag[k], name.encode("ascii"), rs.pos[lo + k], 60 if k % 7 else 3,
                                                                                              c.encode("ascii"), seq[k, :q].tobytes(), qual[k, :q].tobytes(), tail[k].encode("ascii")))
                fh.write(b"".join(lines))
                n_lines += hi - lo
    return n_lines


def _bgzf_piece(args):
    path, at, n = args
    with open(path, "rb") as fh:
        fh.seek(at)
        text = fh.read(n)
    return b"".join(samio._bgzf_block(text[k:k + 0xff00], 6) for k in range(0, len(text), 0xff00))


def _gzip_piece(args):
    path, at, n = args
    with open(path, "rb") as fh:
        fh.seek(at)
        text = fh.read(n)
    comp = zlib.compressobj(6, zlib.DEFLATED, 31)
    return comp.compress(text) + comp.flush()


def write_compressed(sam, bgzf_path, gzip_path, workers=15):
    """The text of ``sam`` as BGZF (level 6, payloads of 0xff00 bytes, the EOF marker) and as gzip (a member per 256 MiB of text).
    The workers are fresh processes (``spawn``), and ``main`` calls this before it opens its context: none of them ever sees the GPU."""
    size = os.path.getsize(sam)
    with multiprocessing.get_context("spawn").Pool(workers) as pool:
        step = 0xff00 * 256
        with open(bgzf_path, "wb") as fh:
            for piece in pool.imap(_bgzf_piece, [(sam, at, step) for at in range(0, size, step)], chunksize=4):
                fh.write(piece)
            fh.write(samio._BGZF_EOF)
        step = 256 << 20
        with open(gzip_path, "wb") as fh:
            for piece in pool.imap(_gzip_piece, [(sam, at, step) for at in range(0, size, step)]):
                fh.write(piece)


def timing_split(make, ctx):
    """One more decode under SPL_BAM_TIMING, the library's stderr caught: -> its lines about this decode."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["SPL_BAM_TIMING"] = "1"
        try:
            src = make()
            src.decode_on_device(ctx)
            src.wait_all()
            src.close()
        finally:
            del os.environ["SPL_BAM_TIMING"]
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        return [line for line in tmp.read().decode("utf-8", "replace").split("\n") if "SAM text" in line]


def best_of(make, ctx, runs=3):
    """A warm-up, then the best of ``runs``: seconds of decode_on_device on a fresh object -> (seconds, records, taken on the device)."""
    best, n, on = None, 0, False
    for rep in range(runs + 1):
        src = make()
        t = time.perf_counter()
        on = src.decode_on_device(ctx)
        src.wait_all()
        dt = time.perf_counter() - t
        n = src.n_records
        src.close()
        if rep:
            best = dt if best is None else min(best, dt)
    return best, n, on


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", default="2000000,20000000")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = []

    def say(msg):
        print(msg, flush=True)
        out.append(msg)
    work = args.dir or tempfile.mkdtemp(prefix="sam_rate_")
    for n_reads in [int(v) for v in args.reads.split(",")]:
        sam, bam = os.path.join(work, "s%d.sam" % n_reads), os.path.join(work, "s%d.bam" % n_reads)
        bgz, gzp = sam + ".bgzf.gz", sam + ".gz"
        free = os.statvfs(work).f_bavail * os.statvfs(work).f_frsize
        if free < 600 * n_reads:
            say("%d reads: skipped, %s has %.1f GB free and the four files need about %.1f" % (n_reads, work, free / 1e9, 600 * n_reads / 1e9))
            continue
        # ---- the four files first, with no context open: the compressing workers are started while this process has no GPU
        t = time.perf_counter()
        wl = synth.Workload("arabidopsis", n_reads=n_reads, seed=5)
        names, lengths = wl.genome.chrom_names, wl.genome.chrom_lengths
        n_lines = write_sam_like_an_aligner(sam, names, lengths, wl.reads)
        native.write_bam(bam, names, lengths, wl.reads, seq_mode=1)
        text_bytes, bam_bytes = os.path.getsize(sam), os.path.getsize(bam)
        say("%d reads: SAM %.3f GB (%.0f B a line), BAM %.3f GB, written in %.0f s" % (n_lines, text_bytes / 1e9, text_bytes / n_lines, bam_bytes / 1e9, time.perf_counter() - t))
        t = time.perf_counter()
        write_compressed(sam, bgz, gzp)
        say("  the text compressed: BGZF (level 6, payloads of 0xff00) %.3f GB = 1/%.2f of the text, gzip %.3f GB; written in %.0f s"
            % (os.path.getsize(bgz) / 1e9, text_bytes / os.path.getsize(bgz), os.path.getsize(gzp) / 1e9, time.perf_counter() - t))
        del wl
        with native.Context(args.device) as ctx:
            t_sam, n_sam, on_sam = best_of(lambda: native.SamFile(sam), ctx)
            floor = text_bytes / (LINK_GBS * 1e9)
            say("  SAM text on the %s: %.4f s until the references are complete = %.2f GB/s of text, %.1f M lines/s; the link's floor at %.0f GB/s is %.4f s (x%.2f)"
                % ("GPU" if on_sam else "HOST (declined or no memory)", t_sam, text_bytes / t_sam / 1e9, n_sam / t_sam / 1e6, LINK_GBS, floor, t_sam / floor))
            t_of = {}
            for form, path in (("BGZF", bgz), ("gzip", gzp)):
                t_z, n_z, on_z = best_of(lambda: native.SamFile(path), ctx)
                t_of[form] = t_z
                say("  SAM text, %s, on the %s: %.4f s = %.2f GB/s of inflated text (x%.2f of the plain text's time, file bytes at the link's rate: %.4f s); %d records: %s"
                    % (form, "GPU" if on_z else "HOST", t_z, text_bytes / t_z / 1e9, t_z / t_sam, os.path.getsize(path) / (LINK_GBS * 1e9), n_z, n_z == n_sam))
            for line in timing_split(lambda: native.SamFile(bgz), ctx):
                say("    " + line)
            t_bam, n_bam, on_bam = best_of(lambda: native.BamFile(bam, defer=True), ctx)
            say("  BAM of the same reads on the %s: %.4f s (%.2f GB/s of file); %d records both ways: %s" % ("GPU" if on_bam else "HOST", t_bam, bam_bytes / t_bam / 1e9, n_bam,
                                                                                                          n_bam == n_sam))
        if n_reads <= 2_000_000:
            for what, path, t_gpu in (("the plain text", sam, t_sam), ("the BGZF text", bgz, t_of["BGZF"]), ("the gzip text", gzp, t_of["gzip"])):
                t = time.perf_counter()
                samio.read_sam(path)
                t_py = time.perf_counter() - t
                say("  the Python reader (samio.read_sam, what -B ran before) on %s: %.2f s = %.0f k lines/s (x%.1f of the GPU's time for that file)"
                    % (what, t_py, n_lines / t_py / 1e3, t_py / t_gpu))
        for path in (sam, bam, bgz, gzp):
            os.remove(path)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
