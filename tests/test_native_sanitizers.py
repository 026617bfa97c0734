"""AddressSanitizer + UBSan (and ThreadSanitizer) builds of host code, each a stand-alone program: the BAM reader/writer, and the
readers and writers of text with the `combine` walk and the host packer on the corpus of textcases.py (GPU sanitizers are not
available on the pool; these are the CPU builds the task allows)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bam_reader_writer_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "bam_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "native", "bam_asan_driver.cpp"), os.path.join(ROOT, "spliser_amd", "csrc", "bam_reader.cpp"),
           "-o", exe, "-lz", "-ldl"]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, str(tmp_path), "200000"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = out.stdout.decode("utf-8", "replace")
    assert out.returncode == 0, text
    assert "ERROR: AddressSanitizer" not in text and "runtime error" not in text, text
    assert text.startswith("ok:")


@pytest.mark.parametrize("batch_blocks", ["1", "32"])
def test_bam_decoder_under_thread_sanitizer(tmp_path, batch_blocks):
    """The decoder hands batches from its workers to the committing thread without a lock (state word per ring slot, frontier
    counter, block directory growing beside it): ThreadSanitizer on the same driver, small batches included (every batch then
    starts inside a record and the ring turns over thousands of times)."""
    exe = str(tmp_path / "bam_tsan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread",
           os.path.join(ROOT, "tests", "native", "bam_asan_driver.cpp"), os.path.join(ROOT, "spliser_amd", "csrc", "bam_reader.cpp"),
           "-o", exe, "-lz", "-ldl"]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if built.returncode != 0:
        pytest.skip("no ThreadSanitizer runtime in this image: " + built.stdout.decode("utf-8", "replace")[-200:])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", SPL_BAM_BATCH_BLOCKS=batch_blocks)
    out = subprocess.run([exe, str(tmp_path), "60000"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    text = out.stdout.decode("utf-8", "replace")
    assert out.returncode == 0 and "ThreadSanitizer" not in text, text[-3000:]
    assert text.startswith("ok:")


# ---- the readers and writers of text, the combine walk and the host packer (tests/native/text_asan_driver.cpp) ---------------------
TEXT_SOURCES = [os.path.join(ROOT, "tests", "native", "text_asan_driver.cpp")] + [os.path.join(ROOT, "spliser_amd", "csrc", s)
                                                                                   for s in ("spl_host.cpp", "spl_combine.cpp", "spl_pack.cpp")]


def _build_text_driver(exe, sanitize):
    """The driver and the three sources it stands on, each compiled on its own (side by side), then linked.  -> (ok, output)"""
    flags = ["g++", "-std=c++17", "-O1", "-g"] + sanitize + ["-pthread"]
    objs = [exe + ".%d.o" % k for k in range(len(TEXT_SOURCES))]
    jobs = [subprocess.Popen(flags + ["-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for src, obj in zip(TEXT_SOURCES, objs)]
    out = b"".join(j.communicate()[0] for j in jobs)
    if any(j.returncode for j in jobs):
        return False, out.decode("utf-8", "replace")
    link = subprocess.run(flags + objs + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return link.returncode == 0, (out + link.stdout).decode("utf-8", "replace")


def _golden_samples():
    import json
    case = os.path.join(ROOT, "tests", "golden", "combine_a")
    with open(os.path.join(case, "combine_manifest.json")) as fh:
        manifest = json.load(fh)
    return {v: [os.path.join(case, "sample%d" % k, "expected.%s.tsv" % v) for k in range(manifest["n_samples"])] for v in sorted(manifest["variants"])}


def _line(kind, name, rc, rows, crc):
    return "%s\t%s\t%d\t%d\t%08x" % (kind, name, rc, rows, crc)


def _expected_line(job, work):
    """What the driver prints for a job, through the ordinary library."""
    import numpy as np
    import textcases as tc
    from spliser_amd import native
    kind, name, paths = job[0], job[1], job[2:]
    if kind in ("bed", "gff"):
        try:
            cols = (native.read_gff_genes if kind == "gff" else native.read_bed_columns)(paths[0])
        except native.SpliserNativeError as err:
            return [_line(kind, name, err.code, 0, 0)]
        if cols is None:
            return [_line(kind, name, -5, 0, 0)]
        return [_line(kind, name, 0, cols.chrom.shape[0], tc.checksum(tc.columns_text(cols, kind == "gff")))]
    if kind == "tsv":
        crc, rows, out = 0, 0, os.path.join(work, "library.combined.tsv")
        for gene, shallow, cryptic in tc.COMBINE_RUNS:
            try:
                walk = native.Combine(list(paths))
            except native.SpliserNativeError as err:
                return [_line(kind, name, err.code, 0, 0)]
            with walk:
                rows = walk.rows(len(paths) - 1)
                chroms = tc.first_appearance(walk.region_runs())
                if shallow is not None and gene != "All":
                    walk.keep_gene(gene)
                skipped = walk.merge(chroms, cryptic, gene, shallow if shallow is not None else None)
                for idx in range(len(paths)):
                    for _, t in walk.tables(idx):
                        walk.answers(idx, t["site"], np.zeros(len(t["site"]), np.uint32), np.zeros(len(t["site"]), np.uint32))
                walk.write(out, ["S%d" % k for k in range(len(paths))], cryptic)
                crc = tc.checksum(("sites %d %d skipped %d\n" % (walk.n_sites, walk.n_gap_sites, len(skipped))).encode(), crc)
            with open(out, "rb") as fh:
                crc = tc.checksum(fh.read(), crc)
        return [_line(kind, name, 0, rows, crc)]
    if kind == "fixed":       # Python's own formatting: the sanitizer build against "{0:.3f}".format, not against the library
        values = np.fromfile(paths[0], np.float64).tolist()
        return [_line(kind, name, 0, len(values), tc.checksum("".join(("{0:.%df}\n" % d).format(x) for x in values for d in tc.FIXED_DIGITS).encode()))]
    if kind == "repr":
        values = np.fromfile(paths[0], np.float64).tolist()
        return [_line(kind, name, 0, len(values), tc.checksum("".join(repr(x) + "\n" for x in values).encode()))]
    if kind == "pack":
        raw = np.fromfile(paths[0], np.uint8)
        n = int(raw[:8].view(np.int64)[0])
        pos, at = raw[8:8 + 4 * n].view(np.int32), 8 + 4 * n
        flag, at = raw[at:at + 2 * n].view(np.uint16), at + 2 * n
        off, at = raw[at:at + 4 * (n + 1)].view(np.uint32), at + 4 * (n + 1)
        desc, rec, wide = native.pack_host(native.ReadArrays(pos.copy(), flag.copy(), off.copy(), raw[at:].view(np.uint32).copy()), threads=3)
        return [_line(kind, name, 0, len(desc), tc.checksum(desc.tobytes() + rec.tobytes() + wide.tobytes()))]
    if kind == "search":
        lines = []
        q_pos = [p for p in tc.GENE_QUERY_POS for _ in tc.GENE_QUERY_STRANDS]
        q_strand = np.frombuffer(tc.GENE_QUERY_STRANDS * len(tc.GENE_QUERY_POS), np.uint8)
        for table, left, right, strand in tc.GENE_TABLES:
            for stranded in (0, 1):
                got = native.gene_search(np.array(left, np.int64), np.array(right, np.int64), np.frombuffer(strand, np.uint8), np.array(q_pos, np.int64), q_strand, stranded)
                text = "".join("%d," % v for v in np.asarray(got).tolist())
                lines.append(_line(kind, table + ("_stranded" if stranded else "_unstranded"), 0, len(q_pos), tc.checksum(text.encode())))
        return lines
    assert kind == "writers"
    lines = [_line("append", "cryptic" if c else "plain", 0, 3, tc.checksum(tc.APPEND_MANY_TEXT[c])) for c in (False, True)]
    path = os.path.join(work, "library.bedgraph")
    for chrom, start, end, depth, per_million_of in tc.BEDGRAPH_RUNS:
        native.bedgraph_append(path, chrom, start, end, depth, per_million_of)
    with open(path, "rb") as fh:
        lines.append(_line("bedgraph", "runs", 0, 5, tc.checksum(fh.read())))
    return lines


def _pack_file(path, records):
    import numpy as np
    from spliser_amd import samio
    reads = samio.ReadSet.from_records(records)
    with open(path, "wb") as fh:
        fh.write(np.int64(reads.n).tobytes() + np.ascontiguousarray(reads.pos, np.int32).tobytes() + np.ascontiguousarray(reads.flag, np.uint16).tobytes() +
                 np.ascontiguousarray(reads.cig_off, np.uint32).tobytes() + np.ascontiguousarray(reads.cigar, np.uint32)[:int(reads.cig_off[-1])].tobytes())


def _run_text_driver(exe, jobs, work, env, timeout):
    manifest = os.path.join(work, "manifest.tsv")
    with open(manifest, "w") as fh:
        fh.writelines("\t".join(job) + "\n" for job in jobs)
    out = subprocess.run([exe, manifest, work], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    return out.returncode, out.stdout.decode("utf-8", "replace")


def test_text_readers_writers_and_combine_walk_under_asan_ubsan(tmp_path):
    """Every file of the corpus of textcases.py through spl_bed_open / spl_gff_open / spl_combine_open in an ASan + UBSan build, and
    past the parsers: every accessor, the walk, tables, answers and writer of `combine` in eight runs a table (all genes and one,
    shallow and not, cryptic and not), the golden combine samples at full length, the row and bedGraph writers, the gene search,
    the number formatters on the value lists of their own tests, the host packer on its corner CIGARs with 1 and 16 threads.  The
    driver's line for every job -- return code, rows, checksum of what it read or wrote -- must be the ordinary library's: the
    sanitizer build read the same thing, and skipped nothing."""
    import numpy as np
    import textcases as tc
    work = str(tmp_path)
    exe = os.path.join(work, "text_asan")
    ok, log = _build_text_driver(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert ok, log
    corpus = tc.write_corpus(work)
    good = os.path.join(work, "good.SpliSER.tsv")
    jobs = [("search", "tables"), ("writers", "small")]
    np.array(tc.fixed_values(), np.float64).tofile(os.path.join(work, "fixed.f64"))
    np.array(tc.repr_values() + [float("nan")], np.float64).tofile(os.path.join(work, "repr.f64"))
    jobs += [("fixed", "values", os.path.join(work, "fixed.f64")), ("repr", "values", os.path.join(work, "repr.f64"))]
    _pack_file(os.path.join(work, "corner.reads"), tc.PACK_CORNER_RECORDS)
    _pack_file(os.path.join(work, "corner_x300.reads"), tc.PACK_CORNER_RECORDS[:-2] * 300 + tc.PACK_CORNER_RECORDS[-2:])   # four chunks
    _pack_file(os.path.join(work, "empty.reads"), [])
    jobs += [("pack", n, os.path.join(work, n + ".reads")) for n in ("corner", "corner_x300", "empty")]
    for variant, paths in _golden_samples().items():
        jobs.append(("tsv", "golden_" + variant) + tuple(paths))
    for fmt in ("bed", "gff"):
        jobs += [(fmt, name, path) for name, path, _ in corpus[fmt]] + [(fmt, "missing", os.path.join(work, "missing"))]
    jobs += [("tsv", name, good, path) for name, path, _ in corpus["tsv"]] + [("tsv", "missing", good, os.path.join(work, "missing"))]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    code, text = _run_text_driver(exe, jobs, work, env, 600)
    assert code == 0, text[-4000:]
    assert "AddressSanitizer" not in text and "runtime error" not in text, text[-4000:]
    got = text.splitlines()
    assert got[0] == "start" and got[-1] == "done\t%d" % len(jobs)
    got = got[1:]
    want = [line for job in jobs for line in _expected_line(job, work)]
    assert len(want) > 9000
    assert got[:-1] == want, [(g, w) for g, w in zip(got, want) if g != w][:10]
    accepted = {fmt: sum(1 for line in want if line.startswith(fmt + "\t") and line.split("\t")[2] == "0") for fmt in ("bed", "gff", "tsv")}
    assert all(n >= 600 for n in accepted.values()), accepted      # (the driver went past the parsers that often)


def test_combine_parse_walk_and_writers_under_thread_sanitizer(tmp_path):
    """spl_combine_open parses its files on a pool of threads, spl_combine_write and spl_tsv_append_many format on one, the packer
    plans and emits on one: the same driver under ThreadSanitizer, on all golden sample tables at once (21 files, 16 threads) and
    variant by variant, the packer on four chunks with 16 threads, the writers."""
    import textcases as tc
    work = str(tmp_path)
    exe = os.path.join(work, "text_tsan")
    ok, log = _build_text_driver(exe, ["-fsanitize=thread"])
    if not ok:
        pytest.skip("no ThreadSanitizer runtime in this image: " + log[-200:])
    samples = _golden_samples()
    everything = tuple(p for paths in samples.values() for p in paths)
    assert len(everything) >= 8
    _pack_file(os.path.join(work, "corner_x300.reads"), tc.PACK_CORNER_RECORDS[:-2] * 300 + tc.PACK_CORNER_RECORDS[-2:])
    jobs = [("tsv", "all_golden_samples") + everything] + [("tsv", "golden_" + v) + tuple(p) for v, p in samples.items()]
    jobs += [("pack", "corner_x300", os.path.join(work, "corner_x300.reads")), ("writers", "small")]
    code, text = _run_text_driver(exe, jobs, work, dict(os.environ, TSAN_OPTIONS="halt_on_error=1"), 600)
    assert code == 0 and "ThreadSanitizer" not in text, text[-3000:]
    got = text.splitlines()
    assert got[0] == "start" and got[-1] == "done\t%d" % len(jobs)
    got = got[1:]
    assert got[:-1] == [line for job in jobs for line in _expected_line(job, work)]
