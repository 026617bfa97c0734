"""bench.py's last stdout line is what the driver parses: it has to be ONE short JSON line whatever the run measured
(round 3's 23 KB line was cut off by the driver's 8 KB tail and nothing of the round's measurement survived)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def canned(n_legs=9, world=1):
    leg = {"workload": "human", "bam": "seq-like", "bam_bytes": 14341234567, "decode": "device", "devices": list(range(world)),
           "wall_s": 0.43312345678, "median_wall_s": 0.4434567891, "first_call_wall_s": 0.80123456, "first_call_device_gb": 13.41, "reads_per_sec": 461234567.891,
           "path": {"what": "prose " * 60, "file_GBps": 33.123456789, "frac_of_pcie": 0.59123456, "pcie_peak_GBps": 56.0},
           "tsv_matches_oracle": True, "cpu_e2e": {"what": "prose " * 40, "reads_per_sec": 40912345.678},
           "what": "prose " * 200, "stages": {"a_s": 0.1, "b_s": 0.2}, "cold_cli_s": 0.7123456, "cold_cli_matches": True,
           "kernels": {"what": "prose " * 50, "table": [{"kernel": "spl_k%d" % k, "calls": 5, "ms": 1.2345678, "bytes": 123456789} for k in range(9)]}}
    return {
        "metric": "splice sites/sec (+ reads/sec) processed", "value": 334710996.8159196, "unit": "splice sites/s",
        "reads_per_sec": 222796814793.11566, "n_gpus": world, "steps": 20, "warmup": 5, "ms_per_step": 0.8976789016742259,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "int32/u32 counters, f64 SSE", "data": "synthetic",
        "config": {"workload": "human: 200000000 reads x 300463 splice sites, 24 chromosomes in 2 shard(s) on rank 0, 150 bp, unstranded",
                   "scale": 1.0, "parallelism": "chromosome/sample shards, no collectives", "seed": 3, "step": "BAM-native arrays resident in HBM -> layout + range + literal + scan/SSE kernels of every shard, barrier between steps"},
        "roofline": {"bound": "hbm", "achieved": 4640.32429710635, "peak": 8000.0, "unit": "GB/s", "frac": 0.5800405371382937,
                     "traffic": 1493338546, "traffic_from": "r03P_traffic.json", "kernel": "spl_count_ranges_kernel",
                     "kernel_ms_avg": 0.4034253999590874, "launches_timed": 40, "algorithmic_bytes_per_launch": 1872024685.5,
                     "layout": {"kernel": "spl_layout_kernel", "kernel_ms_avg": 0.6123456789, "launches_timed": 40, "algorithmic_bytes_per_launch": 3120000000.5,
                                "arrays_read": 1870000000.5, "records_written": 1250000000.0, "achieved": 5095.123456, "frac": 0.636890432, "what": "prose " * 20},
                     "range": {"kernel": "spl_count_ranges_kernel", "kernel_ms_avg": 0.4034253999590874, "launches_timed": 40,
                               "algorithmic_bytes_per_launch": 1872024685.5, "achieved": 4640.32429710635, "frac": 0.5800405371382937, "what": "prose " * 20},
                     "count_only": {"what": "prose " * 20, "ms_per_step": 0.8976789016742259, "reads_per_sec": 222796814793.11566, "path_frac": 0.5213514214293551},
                     "range_traffic": 1493338546, "range_traffic_from": "r03P_traffic.json", "second_kernel": "spl_count_ranges_kernel", "fused": True,
                     "two_kernels": {"ms_per_step": 2.3104123456, "layout_kernel_ms_avg": 0.669312345, "range_kernel_ms_avg": 0.388223456, "layout_bytes_per_launch": 3130000000.5,
                                     "same_counters": True, "steps": 10, "what": "prose " * 30, "layout_frac": 0.58528123, "range_frac": 0.60276123, "path_frac": 0.20256123},
                     "grid": 15856, "block": 256, "lds_bytes": 17404,
                     "alone": {"kernel_ms_avg": 0.39, "frac": 0.5949139256781943, "how": "prose " * 20},
                     "path": {"what": "prose " * 20, "achieved": 4170.8, "frac": 0.5213514214293551},
                     "hbm_actual": {"what": "prose " * 20, "GBps": 3701.6, "frac": 0.4627059135813722},
                     "lib_sha16": "c6c68c61bd907ffa", "kernel_src_sha16": "69beb4938a3f2c1f", "ingest_src_sha16": "b8c7ddf82408e0e2"},
        "cpu_baseline": {"value": 69925.73301240719, "unit": "splice sites/s", "reads_per_sec": 46545320.39712524, "cores": 1,
                         "kind": "port", "sample": "prose " * 40, "sample_short": "whole workload, one pass of oracle/spliser_oracle.c, 4.3 s",
                         "all_cores": {"value": 256805.8, "reads_per_sec": 170940063.4, "nproc": 256, "cpu_quota_cores": 16.0,
                                       "threads_used": 16, "threads": "prose " * 20, "seconds": 1.17, "same_counts_as_1_thread": True},
                         "reference_cost_model": {"estimate_seconds": 585.8379056, "label": "prose " * 40},
                         "reference_measured": {"label": "prose " * 40, "cases": [{"name": "x", "reads": 1}] * 4}},
        "parity": {"reads": 200000000, "sites": 300463, "bit_exact_vs_oracle": True, "of": "the last timed step", "checked": "prose " * 10},
        "e2e": [dict(leg) for _ in range(n_legs)],
        "combine": {"line": {"workload": "combine6: 6 x 20 M reads", "process_s": 1.234567, "combine_s": 2.345678, "parse_s": 0.3,
                             "merge_s": 0.4, "gapfill_s": 0.5, "write_s": 0.6, "queries": 123456, "rows": 1500000, "matches_oracle": True},
                    "what": "prose " * 100},
        "other_steps": [{"workload": "mouse_stranded fr+cryptic", "reads": 100000000, "sites": 229000, "shards": 2, "stranded": "fr", "cryptic": True, "fused": True,
                         "ms_per_step": 1.0871234, "reads_per_sec": 9.2e10, "kernel_ms_avg": 0.48412345, "frac": 0.2421234, "path_frac": 0.2151234, "bit_exact_vs_oracle": True},
                        {"workload": "arabidopsis", "reads": 20000000, "sites": 180000, "shards": 1, "stranded": None, "cryptic": False, "fused": True,
                         "ms_per_step": 0.3011234, "reads_per_sec": 6.6e10, "kernel_ms_avg": 0.2211234, "frac": 0.2101234, "path_frac": 0.1561234, "bit_exact_vs_oracle": True},
                        {"workload": "human clipped30", "reads": 200000000, "sites": 300463, "shards": 2, "stranded": None, "cryptic": False, "fused": True,
                         "ms_per_step": 2.2011234, "reads_per_sec": 9.1e10, "kernel_ms_avg": 1.0211234, "frac": 0.2301234, "path_frac": 0.2101234, "bit_exact_vs_oracle": True}],
        "imbalance": None if world == 1 else {"reads_per_rank": [25000000] * world, "seconds_per_rank": [0.123456] * world,
                                              "max_over_mean_reads": 1.2345678},
        "literal_kernel_reads": 41234, "gen_seconds": 12.3, "upload_seconds": 1.2}


def check(text, want_legs):
    assert "\n" not in text
    assert len(text.encode("utf-8")) < bench.LINE_LIMIT, len(text)
    d = json.loads(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in d["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in d["cpu_baseline"], k
    assert d["config"]["workload"].startswith("human")
    assert "model" not in d["config"]
    assert d["parity"]["bit_exact_vs_oracle"] is True
    assert len(d["e2e"]) == want_legs
    for leg in d["e2e"]:
        assert all(not isinstance(v, (dict, list)) for v in leg.values()), leg
    return d


def test_compact_line_is_short_and_parses():
    d = check(bench.compact_line(canned(n_legs=7)), 7)
    assert abs(d["value"] - 334710996.8159196) / 334710996.8159196 < 1e-4       # (5 significant digits)
    assert d["e2e"][0]["frac_of_pcie"] == 0.59123 and d["e2e"][0]["cpu_e2e_reads_per_sec"] == 40912000.0
    assert d["combine"]["matches_oracle"] is True
    assert d["roofline"]["fused"] is True and d["roofline"]["two_kernels"]["same_counters"] is True
    assert "what" not in d["roofline"]["two_kernels"] and d["e2e"][0]["first_call_device_gb"] == 13.41
    # the other configurations' resident steps ride in the line: config 5's shape, config 2, the clipped sample
    assert [o["workload"] for o in d["other_steps"]] == ["mouse_stranded fr+cryptic", "arabidopsis", "human clipped30"]
    assert all(o["bit_exact_vs_oracle"] is True and o["ms_per_step"] and o["frac"] for o in d["other_steps"])


def test_compact_line_eight_ranks():
    d = check(bench.compact_line(canned(n_legs=4, world=8)), 4)
    assert len(d["imbalance"]["reads_per_rank"]) == 8


def test_compact_line_sheds_before_it_breaks():
    text = bench.compact_line(canned(n_legs=30))
    assert len(text) < bench.LINE_LIMIT
    d = json.loads(text)
    assert d["roofline"]["frac"] and d["cpu_baseline"]["value"] and d["e2e_dropped_for_length"] > 0


def test_no_baseline_no_e2e():
    out = canned(0)
    out["cpu_baseline"], out["e2e"], out["parity"] = None, None, None
    d = json.loads(bench.compact_line(out))
    assert d["cpu_baseline"] is None and d["e2e"] is None


def test_emit_prints_the_compact_line_last(capsys, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    bench.emit(canned(n_legs=5))
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 2 and lines[0].startswith("bench_detail {")
    check(lines[-1], 5)
    with open(tmp_path / "bench_detail.json") as fh:
        assert json.load(fh)["e2e"][0]["kernels"]["table"]


def test_the_committed_traffic_measurement_is_of_these_kernel_sources():
    """bench.py quotes `roofline.traffic` (HBM bytes per launch by the PMC counters) from profiles/*_traffic.json only when the file was
    measured with the kernel sources it runs (kernel_src_sha16: comments and white space aside).  A change to spl_kernels.hip,
    spl_device.h, spl_pack.h, spl_classify.h or spl_pack.cpp without a new `tools/prof_round.sh` run leaves the driver's line with
    `traffic: null` -- which is how round 4 nearly went out (an experiment's switch added after the profile run)."""
    import glob
    sha = bench.kernel_src_sha16()
    have = []
    for path in glob.glob(os.path.join(ROOT, "profiles", "r[0-9]*_traffic.json")):
        with open(path) as fh:
            t = json.load(fh)
        if t.get("workload") == "human":
            have.append(t.get("kernel_src_sha16"))
    assert sha in have, "no profiles/*_traffic.json for the human workload was measured with the current kernel sources (%s): run tools/prof_round.sh" % sha


def _same_workload(a, b):
    for x, y in zip(a.junctions, b.junctions):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert len(a.reads) == len(b.reads) and a.n_reads == b.n_reads and a.genome.chrom_names == b.genome.chrom_names
    for ra, rb in zip(a.reads, b.reads):
        for f in ("pos", "flag", "cig_off", "cigar"):
            assert getattr(ra, f).dtype == getattr(rb, f).dtype and np.array_equal(getattr(ra, f), getattr(rb, f)), f
        assert ra.max_end == rb.max_end


@pytest.mark.parametrize("name,scale,over", [("arabidopsis", 0.01, {}), ("mouse_stranded", 0.002, {"n_genes": 400})])
def test_generate_workload_is_synth_workload(name, scale, over):
    """bench.py's sample generator (per-batch junction tables, chromosomes merged on threads) gives synth.Workload's sample, array
    for array -- in several batches, on several worker processes, paired flags included."""
    from spliser_amd import synth
    want = synth.Workload(name, scale=scale, seed=7, batch=40000, workers=3, **over)
    got = bench.generate_workload(name, scale, 7, 3, over, batch=40000)
    assert len(want.junctions[0]) > 100
    _same_workload(want, got)
    _same_workload(want, bench.generate_workload(name, scale, 7, 1, over, batch=40000))


def _dump_case():
    from spliser_amd import sites, synth
    wl = synth.Workload("arabidopsis", scale=0.002, seed=9, workers=1)
    table = sites.SiteTable(is_stranded=False)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        bed = os.path.join(tmp, "j.bed")
        synth.write_bed(bed, wl.genome.chrom_names, wl.junctions)
        table.add_bed(bed)
    table.find_competitors()
    items = [(c, table.chrom_arrays(c), wl.reads[i]) for i, c in enumerate(wl.genome.chrom_names) if table.chrom_arrays(c).n]
    return items


def test_dump_outputs_writes_the_last_steps_arrays_by_chromosome(tmp_path):
    """--dump-outputs: every array a caller of the step receives, as float64 .npy, chromosome by chromosome in the sample's order
    whatever the shards' packing; past the size limit, the same seeded sample every time."""
    from spliser_amd import shard
    items = _dump_case()
    assert len(items) > 2
    # two packings of the same chromosomes: one shard each, in reverse order
    for shards in (shard.pack(items, concat_reads=False), [shard.pack([it], concat_reads=False)[0] for it in reversed(items)]):
        counts, sses = [], []
        for sh in shards:
            n, n_e = sh.site_rows[-1][1], sh.edge_rows[-1][1]
            base = np.zeros(n, np.int64)
            for chrom, (r0, r1), _ in zip(sh.chroms, sh.site_rows, sh.edge_rows):
                base[r0:r1] = [k for k, it in enumerate(items) if it[0] == chrom][0] * 100000 + np.arange(r1 - r0)
            ebase = np.zeros(n_e, np.int64)
            for chrom, _, (e0, e1) in zip(sh.chroms, sh.site_rows, sh.edge_rows):
                ebase[e0:e1] = [k for k, it in enumerate(items) if it[0] == chrom][0] * 100000 + np.arange(e1 - e0)
            counts.append((base.astype(np.uint32), (base + 1).astype(np.uint32), ebase.astype(np.uint32)))
            sses.append((base + 2, base + 3, base + 0.25, base + 0.5))
        out = tmp_path / ("d%d" % len(shards))
        rows = bench.dump_outputs(str(out), items, shards, counts, sses)
        n_sites = sum(arr.n for _, arr, _ in items)
        want = np.concatenate([k * 100000 + np.arange(arr.n) for k, (_, arr, _) in enumerate(items)]).astype(np.float64)
        assert rows["beta1"] == n_sites and rows["double_counts"] == sum(int(arr.part_off[-1]) for _, arr, _ in items)
        for name, add in zip(bench.DUMP_NAMES, (0, 1, None, 2, 3, 0.25, 0.5)):
            a = np.load(str(out / (name + ".npy")))
            assert a.dtype == np.float64
            if add is not None:
                assert np.array_equal(a, want + add), name
    small = bench.dump_outputs(str(tmp_path / "cut"), items, shards, counts, sses, limit=8 * 7 * 200)
    again = bench.dump_outputs(str(tmp_path / "cut2"), items, shards, counts, sses, limit=8 * 7 * 200)
    assert small == again and max(small.values()) < n_sites
    total = 0
    for name in bench.DUMP_NAMES:
        a, b = np.load(str(tmp_path / "cut" / (name + ".npy"))), np.load(str(tmp_path / "cut2" / (name + ".npy")))
        assert np.array_equal(a, b)
        total += os.path.getsize(str(tmp_path / "cut" / (name + ".npy")))
    assert total <= 8 * 7 * 200
