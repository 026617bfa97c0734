"""``flagstat`` -- the library size without a second tool: samtools flagstat's sixteen counters from the decode of the BAM.

Not part of SpliSER v0.1.8: its README (README.md:234) sends the user to ``samtools flagstat`` for the ``Library_size`` column of
the diffSpliSER target file, "the number of mapped reads in your bam files" -- a second pass over the same file with a second
tool.  Here the decode counts while it walks the records (``spl_bam_set_flagstat``: the device's record scan leaves sixteen
counters a BGZF block, a kernel adds up the blocks the host has accepted; the host decoder's threads count into their own), every
record of the file, placed or not; under a read filter, the records of the pre-filtered file.

The text is samtools' layout as of 1.13, restated from its documentation; parity with the tool itself is not pinned by a test
(DESIGN.md section 9): the definition of the counters is ``spl_flagstat.h``.
"""
from . import native, process as _process

SUFFIX = ".flagstat.txt"
LABELS = native.FLAGSTAT_LABELS
TOTAL, PRIMARY, MAPPED, PRIMARY_MAPPED, PAIRED, PROPER, SINGLETONS = 0, 1, 6, 7, 8, 11, 13
_PERCENT_OF = {MAPPED: TOTAL, PRIMARY_MAPPED: PRIMARY, PROPER: PAIRED, SINGLETONS: PAIRED}     # (line: its denominator)


def _percent(n, d):
    return "%.2f%%" % (100.0 * n / d) if d else "N/A"


def format_lines(counts):
    """``counts``: (16, 2) -- per category the QC-passed and QC-failed records -> the sixteen lines, without newlines."""
    lines = []
    for c, label in enumerate(LABELS):
        p, f = int(counts[c][0]), int(counts[c][1])
        line = "%d + %d %s" % (p, f, label)
        if c in _PERCENT_OF:
            d = _PERCENT_OF[c]
            line += " (%s : %s)" % (_percent(p, int(counts[d][0])), _percent(f, int(counts[d][1])))
        lines.append(line)
    return lines


def write_and_log(path, counts, log):
    with open(path, "w") as out:
        out.write("\n".join(format_lines(counts)) + "\n")
    log("Library size: %d mapped reads (%d primary)" % (int(counts[MAPPED][0]), int(counts[PRIMARY_MAPPED][0])))


def flagstat(inBAM, outputPath, devices=(0,), threads=0, gpuDecode=None, minMapQ=0, requireFlags=0, excludeFlags=0, log=None, anyOrder=False):
    """Writes ``outputPath`` (the sixteen lines) and returns the counters, (16, 2).  ``minMapQ`` / ``requireFlags`` /
    ``excludeFlags``: the read filter of ``process`` -- the counters of the pre-filtered file.  ``gpuDecode``: as for ``process``.
    ``anyOrder``: the BAM may be in any record order and stays on the GPU all the same (``process``); the counters do not depend on it.

    The decode is the NORMAL one with its reads dropped: the blocks are inflated, scanned and their records extracted as for
    ``process``, and nothing is counted against sites.  A decode that stops after the scan would save the extraction kernel's
    share of the decode (about a tenth of it) at the price of a second path through the window loop; it is not arranged."""
    log = _process.logger(log)
    options = _process.DecodeOptions(_process.read_filter(minMapQ, requireFlags, excludeFlags), flagstat=True, any_order=bool(anyOrder))
    with _process.decoding(inBAM, devices, gpuDecode, threads, options, log=log) as source:
        counts = source.flagstat()
        if anyOrder:
            _process.log_any_order(source, log)
        if gpuDecode is not False and source.decline_reason():
            log("  (the alignment file was decoded on host threads, not on the GPU: %s)" % source.decline_reason())
        _process.log_filter(source, options.read_filter, log)
    write_and_log(outputPath, counts, log)
    return counts
