"""How a wave of ``spl_exon_count_fragments`` adds its 64 reads' fragments to the counts: the kernel's body -- the sides and the
verdict of spl_exonfragment_rule.h, then the MERGE of the two mates' walks as the source of ``splexon::wave_commit`` -- built for
the host against tests/hostsim/wave_emul.h (a wave = 64 fibers, every cross-lane primitive a checked rendezvous) and held against
the yardstick of ``exonfragcases.py``: the bins' sums, the four verdict counters, and the number of 64-bit adds under the round rule
with silent lanes offering nothing.  The reference has no such step: it counts no exon bins."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import exoncases as X
import exonfragcases as F
import genecases as G
import matecases as M
from spliser_amd import exoncounts as xc, samio

HERE = os.path.dirname(os.path.abspath(__file__))
BYTE = {"+": 43, "-": 45, ".": 46}


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(HERE, "hostsim", "libexonfragment_wave_host.so")
    csrc = os.path.join(HERE, "..", "spliser_amd", "csrc")
    srcs = [os.path.join(HERE, "hostsim", "exonfragment_wave_host.cpp"), os.path.join(HERE, "hostsim", "wave_emul.h")] + \
           [os.path.join(csrc, h) for h in ("spl_exonfragment_rule.h", "spl_exoncount_rule.h", "spl_mate_rule.h", "spl_genecount_rule.h", "spl_exoncount_wave.h", "spl_genecount_wave.h",
                                            "spl_wave.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
    return ctypes.CDLL(so)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _arrays(features):
    return (np.array([f[0] for f in features], np.int64), np.array([f[1] for f in features], np.int64), np.array([BYTE[f[2]] for f in features], np.uint8),
            np.array([f[3] for f in features], np.int64))


def run(lib, rs, mate, a, b, bin_gene, stranded):
    """-> (counts[n_bins] + tallies[4], the adds as a list of (bin, value) in the order they were made)."""
    none = (np.zeros(0, np.int32), np.zeros(0, np.uint32))
    a, b = a or none, b or none
    pos, flag, off, cigar = rs.pos.astype(np.int32), rs.flag.astype(np.uint16), rs.cig_off.astype(np.uint32), np.concatenate((rs.cigar.astype(np.uint32), np.zeros(1, np.uint32)))
    mate, bin_gene = np.asarray(mate + [0], np.uint32), np.asarray(list(bin_gene) + [0], np.uint32)
    n_bins = bin_gene.shape[0] - 1
    counts, tallies = np.zeros(max(n_bins, 1), np.uint64), np.zeros(4, np.uint64)
    adds, n_adds = np.zeros(2 * 200000, np.uint64), ctypes.c_uint64(0)
    rc = lib.exonfragment_wave_run(ctypes.c_int64(rs.n), _ptr(pos), _ptr(flag), _ptr(off), _ptr(cigar), ctypes.c_int64(rs.cigar.shape[0]), _ptr(mate), ctypes.c_int32(0),
                                   ctypes.c_int(stranded), ctypes.c_int64(a[0].shape[0]), _ptr(a[0]), _ptr(a[1]), ctypes.c_int64(b[0].shape[0]), _ptr(b[0]), _ptr(b[1]),
                                   ctypes.c_uint32(n_bins), _ptr(bin_gene), _ptr(counts), _ptr(tallies), _ptr(adds), ctypes.c_uint64(len(adds) // 2), ctypes.byref(n_adds))
    assert rc == 0, "the wave broke a rule of the emulator (%d)" % rc
    assert n_adds.value <= len(adds) // 2
    return counts[:n_bins].tolist() + tallies.tolist(), [(int(x), int(v)) for x, v in adds[:2 * n_adds.value].reshape(-1, 2).tolist()]


def both(lib, records, keys, features, length, stranded):
    """The emulated waves against the yardstick: the sums, and the adds of the round rule.  -> (the yardstick's results, the adds)."""
    rs = samio.ReadSet.from_records(records)
    mate = M.mate_table_of(rs, keys)[0]
    labels = {w: X.labels_of_features(features, length, w) for w in "+-"} if stranded else X.labels_of_features(features, length)
    a, b, (gene, start, end) = xc.exon_maps(*_arrays(features), stranded=bool(stranded))
    bins = list(zip(start.tolist(), end.tolist(), gene.tolist()))
    results = F.numbered(F.fragment_results(rs, keys, labels, stranded, mate=mate), {key: k for k, key in enumerate(bins)})
    sums, adds = run(lib, rs, mate, a, b, gene, stranded)
    assert sums == F.counts_of(results, None, len(bins))
    assert (len(adds), sum(v for _, v in adds)) == F.adds_of(results)
    return results, adds


@pytest.mark.parametrize("stranded", [0, 1, 2])
def test_generated_paired_content_over_many_waves(lib, stranded):
    rng = np.random.default_rng(20261022)
    features = G.random_features(rng, 2200, 9, 16) + [(2400 + 770 * g + 110 * j, 2480 + 770 * g + 110 * j, "+-."[g], g) for g in range(3) for j in range(7)]
    records, names, _ = M.paired_records(rng, 500, 4800)
    results, adds = both(lib, records, [M.name_key(n) for n in names], features, 6000, stranded)
    verdicts = [v for v, _ in results]
    assert all(verdicts.count(v) > 10 for v in (F.COUNTED, F.NO_FEATURE, F.AMBIGUOUS, F.NOT_COUNTED, F.SILENT)) and len(results) > 64 * 10


@pytest.mark.parametrize("stranded", [0, 1])
@pytest.mark.parametrize("spread", [0, 70])
def test_the_hand_cases_with_silent_lanes(lib, spread, stranded):
    names = sorted(F.HAND_CASES)
    records, keys, where = F.hand_set(names, spread)
    results, _ = both(lib, records, keys, F.HAND_FEATURES, F.HAND_LENGTH, stranded)
    assert [results[w][0] for w in where] == [F.HAND_CASES[n][2 + stranded][0] for n in names]
    assert all(results[w + spread + 1] == (F.SILENT, []) for w in where)


@pytest.mark.parametrize("lead_at", [0, 63])
@pytest.mark.parametrize("name", ["a mate over 70 bins, a one-bin leader", "a leader over 70 bins, a one-bin mate"])
def test_over_70_bins_on_either_mate_beside_one_bin_fragments(lib, name, lead_at):
    """The wave goes on for 75 rounds; the mate's lane is silent throughout."""
    one = "both mates wholly in one bin: + 1, not + 2"
    records, keys = [], []
    for k in range(32):          # 32 fragments of neighbours: a wave
        lead, mate = F.HAND_CASES[name][:2] if 2 * k == lead_at - lead_at % 2 else F.HAND_CASES[one][:2]
        records += [lead, mate]
        keys += [2 * k + 2] * 2
    if lead_at % 2:              # the leader at an odd lane: one filler in front, and its mate is the next wave's lane 0
        records, keys = [F.FILLER] + records, [0] + keys
    results, adds = both(lib, records, keys, F.HAND_FEATURES, F.HAND_LENGTH, 0)
    assert results[lead_at][0] == F.COUNTED and len(results[lead_at][1]) == F.MANY_BINS > 70
    assert sum(1 for x, _ in adds) >= F.MANY_BINS


def test_all_lanes_one_fragment_bin_is_32_adds_of_one(lib):
    """Neighbours that are mates: every second lane is silent and ends the run -- the adds are one per fragment, not one per wave."""
    lead, mate = F.HAND_CASES["both mates wholly in one bin: + 1, not + 2"][:2]
    records, keys = [lead, mate] * 32, [k // 2 * 2 + 2 for k in range(64)]
    results, adds = both(lib, records, keys, F.HAND_FEATURES, F.HAND_LENGTH, 0)
    assert adds == [(0, 1)] * 32
    # ... and leaders first, mates behind them: one add of 32
    records, keys = [lead] * 32 + [mate] * 32, [2 * k + 2 for k in range(32)] * 2
    results, adds = both(lib, records, keys, F.HAND_FEATURES, F.HAND_LENGTH, 0)
    assert adds == [(0, 32)]
