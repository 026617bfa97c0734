"""CPU checks of scancases.py: the plain reference agrees with the host decoder on every legal case, its guessed starts are the true
boundaries except where a case says otherwise, every case reaches the limit it names, and nothing the kernels may read lies
outside the buffer the GPU test allocates.  Families 8 to 10 (windows, contradictions, decoys) go to the card only through this."""
import struct

import numpy as np
import pytest

import scancases as sc
from spliser_amd import native, samio

LEGAL = (1, 2, 3, 4, 5, 6, 11)      # the families that are files the host decoder reads


@pytest.fixture(scope="module")
def built():
    native.build()
    return native.lib()


def write_file(case, path):
    with open(path, "wb") as fh:
        for payload in case.payloads():
            fh.write(samio._bgzf_block(payload, 1))
        fh.write(samio._BGZF_EOF)


def check_reads(bam, case, want_xs=False):
    """The decoder's arrays per reference against reference_extract over the TRUE offsets."""
    names = sc.ref_names(case.n_ref)
    offsets = [o for o in case.offsets if o < case.stream_len]
    n_total = 0
    for t, c in enumerate(names):
        want = sc.reference_extract(case.data, offsets, case.n_ref, t, t + 1, case.filt)
        got = bam.reads(c)
        assert got.n == len(want["pos"]), (case.name, c)
        assert np.array_equal(got.pos, want["pos"]) and np.array_equal(got.flag, want["flag"]), (case.name, c)
        assert np.array_equal(got.cig_off, want["cig_off"]) and np.array_equal(got.cigar, want["cigar"]), (case.name, c)
        assert got.max_end == want["ref_max_end"][t], (case.name, c)
        if want_xs and got.n:
            assert np.array_equal(got.xs, want["xs"]), (case.name, c)
        n_total += got.n
    return n_total


@pytest.mark.parametrize("family", LEGAL)
def test_reference_against_the_host_decoder(built, tmp_path, family):
    seen = set()
    for k, case in enumerate(sc.cases(family)):
        path = str(tmp_path / ("f%d.bam" % k))
        write_file(case, path)
        bam = native.BamFile(path, threads=2, min_mapq=case.filt[0], require_flags=case.filt[1], exclude_flags=case.filt[2], aux_strand=family == 11)
        n_kept = check_reads(bam, case, want_xs=family == 11)
        assert bam.n_records == sum(1 for o in case.offsets if o < case.stream_len)
        scan = sc.reference(case)[0]
        if case.tid_hi == case.n_ref + 1 and case.tid_lo == 0:      # (every record the scan's: its counters are the file's)
            assert bam.filter_counts() == (int(scan["n_drop_flags"].sum()), int(scan["n_drop_mapq"].sum())), case.name
            if sc.extractable(scan):
                assert int(scan["n_placed"].sum()) == n_kept and int(scan["n_all"].sum()) == bam.n_records, case.name
        bam.close()
        seen.add(case.name)
    assert len(seen) == len(sc.cases(family))


@pytest.mark.parametrize("family", (1, 2, 3, 4, 5, 6, 7, 11))
def test_guessed_starts_are_true_boundaries(family):
    """Whole streams of plausible records (the one record without a reference of the header in family 5 lies where no block's first
    boundary is within three records in front of it): every block's start is the first true boundary at or after its first byte --
    except where the 1 MiB reach says there is none to be found -- and every walk arrives where the next block starts."""
    for case in sc.cases(family):
        scan, places, _ = sc.reference(case)
        blocks = case.blocks()
        for b in range(len(scan)):
            u0, u1 = int(blocks["out"][b]), int(blocks["out"][b]) + int(blocks["out_len"][b])
            if u1 <= case.header_end and not u0 == u1 == case.header_end:
                assert scan["start"][b] == u1 == scan["reached"][b]
                continue
            want = sc.true_start(case, max(u0, case.header_end)) if u0 > case.header_end else case.header_end
            if scan["flags"][b] & sc.NO_START:
                assert family == 2 and want + sc.HEAD_BYTES > u0 + sc.REACH, (case.name, b)
                continue
            assert scan["start"][b] == want, (case.name, b, int(scan["start"][b]), want)
            assert scan["reached"][b] == sc.true_start(case, max(u1, want)), (case.name, b)
            assert len(places[b]) == scan["n_placed"][b] <= sc.REC_CAP
        if family != 2 or not np.any(scan["flags"] & sc.NO_START):
            assert sc.extractable(scan)
            want_reason = "not sorted by reference" if case.notes.get("sorted") is False else "a CIGAR parked in a CG tag" if case.notes.get("needs_host") else ""
            assert sc.decline_reason(case, scan) == want_reason, case.name


def test_windows_are_what_they_say():
    """Family 8: with more behind the window, the block whose record runs past it is INCOMPLETE (and NO_START where nothing could be
    chained); without, the same record is CORRUPT where a block walks to it; neither depends on the bytes behind stream_len; in front of the cut record the
    starts are the true boundaries."""
    by_key = {}
    kinds = set()
    for case in sc.cases(8):
        scan, places, far = sc.reference(case)
        assert far <= case.stream_len
        cut = case.notes["cut"]
        inside = cut not in case.offsets
        flags = int(np.bitwise_or.reduce(scan["flags"]))
        if case.more:
            assert not flags & sc.CORRUPT
            if inside:
                assert flags & sc.INCOMPLETE, case.name
        else:
            assert not flags & (sc.INCOMPLETE | sc.NO_START)
            assert not (flags & sc.CORRUPT and not inside), case.name
            reason = sc.decline_reason(case, scan)   # (a cut record is CORRUPT in the block that walks to it, or nobody walks to it: the chain ends short)
            assert bool(reason) == inside and (not flags & sc.CORRUPT or reason == "a record contradicts itself"), case.name
        kinds.add((case.more, flags & (sc.CORRUPT | sc.INCOMPLETE | sc.NO_START)))
        blocks = case.blocks()
        for b in range(len(scan)):
            u0 = int(blocks["out"][b])
            t = sc.true_start(case, u0)
            if u0 > case.header_end and not scan["flags"][b] & sc.NO_START and t + sc.HEAD_BYTES + 3 * 300 <= cut:
                assert scan["start"][b] == t, (case.name, b)
        key = (cut, case.more)
        if key in by_key:
            assert by_key[key][0].tobytes() == scan.tobytes() and by_key[key][1] == places, case.name
        by_key[key] = (scan, places)
    assert kinds >= {(1, sc.INCOMPLETE), (1, sc.INCOMPLETE | sc.NO_START), (0, 0), (0, sc.CORRUPT)}


def test_contradictions_stop_the_walk_at_the_bad_record():
    for case in sc.cases(9):
        scan, _, far = sc.reference(case)
        assert far <= case.stream_len
        bad = case.offsets[case.notes["bad_index"]]
        hit = np.flatnonzero(scan["flags"] & sc.CORRUPT)
        if not case.notes["corrupt"]:
            assert len(hit) == 0 and sc.extractable(scan), case.name
            continue
        assert sc.decline_reason(case, scan) != "", case.name
        if len(case.lens) > 1 and not len(hit):      # (small blocks: the guesses step over the bad record, nobody walks to it, the chain breaks)
            continue
        b = int(hit[0])
        assert scan["reached"][b] == bad, (case.name, b)
        if len(case.lens) == 1:
            assert scan["n_all"][0] == case.notes["bad_index"]


def test_decoys_are_taken_exactly_where_the_case_says():
    for case in sc.cases(10):
        scan, _, _ = sc.reference(case)
        blocks = case.blocks()
        if "decoy_at" in case.notes:
            for b in range(1, len(scan)):
                t = sc.true_start(case, int(blocks["out"][b]))
                assert scan["start"][b] == case.notes["decoy_at"].get(b, t), (case.name, b)
            if case.notes["decoy_at"]:
                b = min(case.notes["decoy_at"])
                assert scan["reached"][b - 1] != scan["start"][b]
                assert sc.decline_reason(case, scan) == case.notes.get("reason", "a guessed record boundary did not hold"), case.name
            else:
                assert sc.decline_reason(case, scan) == ""
        else:       # the tiling of 61: the blocks that begin among the decoys guess a decoy, all others the truth
            lo, hi = case.notes["decoy_from"], case.notes["decoy_to"]
            n_decoy = 0
            for b in range(1, len(scan)):
                u0 = int(blocks["out"][b])
                if u0 <= case.header_end:
                    continue
                t = sc.true_start(case, u0)
                if scan["start"][b] != t:
                    assert lo <= scan["start"][b] < hi and case.offsets[5] < u0 < hi, (case.name, b)
                    n_decoy += 1
            assert n_decoy >= 2


def test_every_case_reaches_the_limit_it_names():
    # family 1: a size word straddling a cut at each of 1, 2 and 3 bytes; cuts at every byte of every record; the header's end in each position
    straddles = set()
    for case in sc.cases(1):
        cuts = set(np.cumsum(case.lens).tolist())
        for o in case.offsets:
            straddles |= {k for k in (1, 2, 3) if o + k in cuts}
        if case.notes["L"] == 1:
            assert cuts >= set(range(case.header_end, case.stream_len))
        how = case.notes["header"]
        H = case.header_end
        blocks = case.blocks()
        ends = (blocks["out"] + blocks["out_len"]).tolist()
        if how == "inside" and case.notes["L"] > 1:
            assert H not in ends
        if how != "inside":
            assert H in ends
        if how == "at_empty":
            assert any(int(o) == H and int(n) == 0 for o, n in zip(blocks["out"], blocks["out_len"]))
        if case.name.endswith("empties"):
            assert case.lens[0] == 0 and case.lens[-1] == 0 and int((case.lens == 0).sum()) >= 3
    assert straddles == {1, 2, 3}
    sizes = [len(r) for r in sc.cases(1)[0].records]
    assert min(sizes) == 37 and sorted(sizes)[len(sizes) * 9 // 10 - 1] <= 150 and len(sizes) == 60
    names = [r[12] for r in sc.cases(1)[0].records]
    assert 1 in names and 255 in names
    # family 2: blocks in which nothing begins, a start beyond the block's end, NO_START exactly where the reach says
    for case in sc.cases(2):
        scan, _, _ = sc.reference(case)
        blocks = case.blocks()
        u1 = blocks["out"] + blocks["out_len"]
        assert np.any((scan["n_all"] == 0) & (scan["start"] >= u1) & (blocks["out"] > case.header_end) & (scan["flags"] == 0)), case.name
        assert np.any(scan["start"] > u1)
        if "big_end" in case.notes:
            end = case.notes["big_end"]
            assert case.notes["big"] > sc.REACH + 128 * 1024
            for b in range(len(scan)):
                u0 = int(blocks["out"][b])
                inside = case.offsets[6] < u0 < end
                assert bool(scan["flags"][b] & sc.NO_START) == (inside and end + sc.HEAD_BYTES > u0 + sc.REACH), (case.name, b)
            edge = end + sc.HEAD_BYTES - sc.REACH            # a block beginning here finds the record behind the large one with its last candidate
            assert (edge in blocks["out"].tolist()) == (case.notes["shift"] == 0)
            assert (edge + case.notes["shift"] in blocks["out"].tolist())
            assert sc.decline_reason(case, scan) == "no record boundary found near a block"
        else:
            assert case.notes["big"] > 200_000 and sc.decline_reason(case, scan) == ""
    # family 3: 1 772 records begin in a block, at its first byte and with a record straddling in
    for case in sc.cases(3):
        scan, places, _ = sc.reference(case)
        full = np.flatnonzero(scan["n_placed"] == 1772)
        assert 1772 <= sc.REC_CAP and len(full) >= 1 and 1772 > 27 * 64
        assert places[int(full[0])][0] == case.notes["straddle"]
    # family 4: the op counts neighbouring in one block, more than 64 placed records in front of them; an end above 2^31
    for case in sc.cases(4):
        scan, places, _ = sc.reference(case)
        b = int(np.argmax(scan["n_ops"]))
        assert scan["n_placed"][b] > 100 and scan["n_ops"][b] > 65535 + 63 + 64 + 65
        n_cig = [struct.unpack_from("<H", r, 16)[0] for r in case.records]
        at = n_cig.index(0, 101)
        assert n_cig[at:at + 6] == [0, 1, 63, 64, 65, 65535]
        want = sc.reference_extract(case.data, case.offsets, 3, 0, 4, (0, 0, 0))
        assert want["ref_max_end"][0] == (1 << 31) - 1 + 100_000_000 - 1 and want["ref_max_end"][2] == (1 << 31) - 1
        assert want["ref_max_end"][1] == 1001 + 61          # (the = and X ops alone put it there)
        assert 0xFFFF in want["flag"].tolist()
    # family 5: three references in one block; the window's counters
    by = {c.name: c for c in sc.cases(5)}
    scan = sc.reference(by["refs/three_in_one"])[0]
    assert (scan["tid_first"][1], scan["tid_last"][1]) == (0, 2) and scan["n_placed"][1] > 12 + 2
    scan = sc.reference(by["refs/window_1_2"])[0]
    assert scan["n_foreign"].sum() == 30 + 30 + 13 and scan["n_foreign_hi"].sum() == 30 + 13 and scan["n_all"].sum() == 12
    assert np.all(scan["n_foreign"][1:] > scan["n_foreign_hi"][1:] - (scan["n_foreign"][1:] == scan["n_foreign_hi"][1:]))
    assert sc.reference(by["refs_down_inside/one"])[0]["flags"][0] == sc.UNSORTED
    scan = sc.reference(by["refs_down_across/two"])[0]
    assert not scan["flags"].any() and scan["tid_first"][1] < scan["tid_last"][0]
    # family 6: every verdict, records that fail both ways among them
    both = 0
    for case in sc.cases(6):
        scan = sc.reference(case)[0]
        for r in case.records:
            tid, pos, _, mapq, _, _, flag = struct.unpack_from("<iiBBHHH", r, 4)
            both += tid >= 0 and pos >= 0 and sc.verdict(case.filt, flag, mapq) == 1 and mapq < case.filt[0]
        if case.filt in ((10, 0, 0), (30, 0x1, 0x400)):
            assert scan["n_drop_mapq"].sum() > 0
        if case.filt != (10, 0, 0) and case.filt != (255, 0, 0):
            assert scan["n_drop_flags"].sum() > 0
    assert both > 0
    # family 7
    for case in sc.cases(7):
        scan = sc.reference(case)[0]
        assert bool(np.any(scan["flags"] & sc.NEEDS_HOST)) == case.notes["needs_host"], case.name
    # family 11: spliced reads of every strand byte; the pad behind the stream spells a strand
    case = sc.cases(11)[0]
    want = sc.reference_extract(case.data, case.offsets, 3, 0, 4, (0, 0, 0))
    assert {0, ord("+"), ord("-")} <= set(want["xs"].tolist())
    assert case.buffer()[case.stream_len:case.stream_len + 4] == b"XSA-" and want["xs"][-1] == 0


@pytest.mark.parametrize("family", sorted(sc.FAMILIES))
def test_nothing_is_read_outside_the_buffer(family):
    """The farthest byte the reference reads, the 36 + 255 bytes a plausibility check may look at from there and the extraction's
    two 16-byte loads lie inside the stream and its pad -- and a block's places fit 16 bits."""
    for case in sc.cases(family):
        scan, places, far = sc.reference(case)
        assert far <= case.stream_len
        assert far + 36 + 255 + 32 <= len(case.buffer())
        assert int(scan["reached"].max()) <= case.stream_len and int(scan["start"].max()) <= case.stream_len
        assert int(case.lens.max()) <= 65536 and int(case.lens.sum()) == case.stream_len
        assert all(p < 65536 for pl in places for p in pl)
        if sc.extractable(scan):
            assert int(scan["n_placed"].max()) <= sc.REC_CAP
