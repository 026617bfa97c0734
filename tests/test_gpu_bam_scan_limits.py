"""The record scan, both extractions (walking and a wave per block, each with and without the strand byte) and the bounds kernel of
spl_inflate.hip on the hand-built streams of scancases.py: every field of every block against the plain reference, every output
array against it and the two extractions against each other, guard areas behind every array; then the same cuts as BGZF files
through the device decoder, which must TAKE what the reference's rule says it must -- a fall-back to the host decoder would hide a
scan that never gets a hard block right.  test_scancases_host.py has shown that the cases are what they say, that the reference
agrees with the host decoder, and that nothing is read outside the buffers allocated here."""
import ctypes

import numpy as np
import pytest

import scancases as sc
from spliser_amd import native
from test_scancases_host import check_reads, write_file

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 256          # bytes behind every output array that must keep their fill
FILL = 0xA5
R0, O0 = 3, 5        # where the first block's records and ops go in the output arrays: not at their beginning


@pytest.fixture(scope="module")
def lib():
    native.build()
    return native.lib()


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def _out(n_bytes):
    return torch.full((n_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")


def _host(t, n_bytes, dt, what):
    raw = t.cpu().numpy()
    assert raw[n_bytes:].tobytes() == bytes([FILL]) * GUARD, "written behind " + what
    return raw[:n_bytes].view(dt)


def run_scan(lib, case):
    """-> (device buffers, scan as BSCAN array, recs as n_blocks x REC_CAP uint16), guards checked."""
    blocks = case.blocks()
    n = len(blocks)
    d_stream, d_blocks = _dev(np.frombuffer(case.buffer(), np.uint8)), _dev(blocks)
    d_scan, d_recs = _out(n * sc.BSCAN.itemsize), _out(n * sc.REC_CAP * 2)
    rc = lib.spl_dev_launch_bam_scan(_p(d_stream), ctypes.c_uint64(case.stream_len), ctypes.c_uint64(case.header_end), ctypes.c_int32(case.n_ref), ctypes.c_int32(case.tid_lo),
                                     ctypes.c_int32(case.tid_hi), _p(d_blocks), ctypes.c_uint32(n), _p(d_scan), ctypes.c_int(case.more), _p(d_recs),
                                     ctypes.c_uint32(case.filt[0]), ctypes.c_uint32(case.filt[1]), ctypes.c_uint32(case.filt[2]), ctypes.c_void_p(0))
    assert rc == 0
    torch.cuda.synchronize()
    scan = _host(d_scan, n * sc.BSCAN.itemsize, sc.BSCAN, "scan")
    recs = _host(d_recs, n * sc.REC_CAP * 2, np.uint16, "recs").reshape(n, sc.REC_CAP)
    return (d_stream, d_blocks, d_recs), scan, recs


def check_scan(case, scan, recs):
    want, places, _ = sc.reference(case)
    for f in sc.BSCAN.names:
        bad = np.flatnonzero(scan[f] != want[f])
        assert len(bad) == 0, "%s: %s of block %d is %d, the reference says %d" % (case.name, f, bad[0], scan[f][bad[0]], want[f][bad[0]])
    for b, mine in enumerate(places):
        k = min(len(mine), sc.REC_CAP)
        assert recs[b, :k].tolist() == mine[:k], (case.name, b)
        assert np.all(recs[b, k:] == FILL * 0x101), (case.name, b)     # (and not a place more)


def run_extract(lib, case, bufs, want_scan, with_recs, with_xs, n_rec, n_ops):
    d_stream, d_blocks, d_recs = bufs
    n = len(want_scan)
    rec_off = R0 + np.concatenate(([0], np.cumsum(want_scan["n_placed"].astype(np.uint64))[:-1])).astype(np.uint64)
    op_off = O0 + np.concatenate(([0], np.cumsum(want_scan["n_ops"].astype(np.uint64))[:-1])).astype(np.uint64)
    d_scan, d_rec_off, d_op_off = _dev(want_scan), _dev(rec_off), _dev(op_off)
    d_pos, d_flag, d_cig_off, d_cigar, d_tid = _out(4 * (R0 + n_rec)), _out(2 * (R0 + n_rec)), _out(4 * (R0 + n_rec + 1)), _out(4 * (O0 + n_ops)), _out(4 * (R0 + n_rec))
    d_xs = _out(R0 + n_rec) if with_xs else None
    d_cig_off[4 * R0:4 * R0 + 4] = torch.from_numpy(np.array([O0], np.uint32).view(np.uint8).copy()).to("cuda:0")
    n_max = case.n_ref + 1
    d_max = torch.zeros(n_max + 8, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    rc = lib.spl_dev_launch_bam_extract(_p(d_stream), ctypes.c_uint64(case.stream_len), ctypes.c_int32(case.n_ref), ctypes.c_int32(case.tid_lo), ctypes.c_int32(case.tid_hi),
                                        _p(d_blocks), ctypes.c_uint32(n), _p(d_scan), _p(d_rec_off), _p(d_op_off), _p(d_pos), _p(d_flag), _p(d_cig_off), _p(d_cigar), _p(d_tid),
                                        _p(d_max), _p(d_recs if with_recs else None), ctypes.c_uint32(case.filt[0]), ctypes.c_uint32(case.filt[1]), ctypes.c_uint32(case.filt[2]),
                                        _p(d_xs), ctypes.c_void_p(0))
    assert rc == 0
    torch.cuda.synchronize()
    got = dict(pos=_host(d_pos, 4 * (R0 + n_rec), np.int32, "pos"), flag=_host(d_flag, 2 * (R0 + n_rec), np.uint16, "flag"),
               cig_off=_host(d_cig_off, 4 * (R0 + n_rec + 1), np.uint32, "cig_off"), cigar=_host(d_cigar, 4 * (O0 + n_ops), np.uint32, "cigar"),
               tid=_host(d_tid, 4 * (R0 + n_rec), np.int32, "tid"))
    if with_xs:
        got["xs"] = _host(d_xs, R0 + n_rec, np.uint8, "xs")
    got["ref_max_end"] = [int(x) for x in d_max.cpu().numpy().view(np.uint64)]
    return got


def check_extract(case, got, want, n_rec, n_ops, how):
    for k, lead in (("pos", R0), ("flag", R0), ("tid", R0), ("cig_off", R0), ("cigar", O0)) + ((("xs", R0),) if "xs" in got else ()):
        a = got[k]
        assert a[:lead].tobytes() == bytes([FILL]) * (lead * a.itemsize), "%s (%s): %s written in front of the first record" % (case.name, how, k)
        assert np.array_equal(a[lead:], want[k]), "%s (%s): %s" % (case.name, how, k)
    assert got["ref_max_end"] == want["ref_max_end"] + [0] * (len(got["ref_max_end"]) - len(want["ref_max_end"])), (case.name, how)


@pytest.mark.parametrize("family", sorted(sc.FAMILIES))
def test_scan_and_extraction_against_the_reference(lib, family):
    n_extracted = 0
    for case in sc.cases(family):
        want_scan, places, _ = sc.reference(case)
        bufs, scan, recs = run_scan(lib, case)
        check_scan(case, scan, recs)
        if not sc.extractable(want_scan):          # (what records_done would not let through is never launched)
            continue
        assert int(want_scan["n_placed"].max()) <= sc.REC_CAP
        blocks = case.blocks()
        offsets = [int(blocks["out"][b]) + p for b, mine in enumerate(places) for p in mine]
        n_rec, n_ops = int(want_scan["n_placed"].sum()), int(want_scan["n_ops"].sum())
        want = sc.reference_extract(case.buffer(), offsets, case.n_ref, case.tid_lo, case.tid_hi, case.filt, cig_off0=O0)
        assert len(want["pos"]) == n_rec and len(want["cigar"]) == n_ops
        results = {}
        for with_recs in (False, True):
            for with_xs in (False, True):
                how = ("wave" if with_recs else "walk") + ("+xs" if with_xs else "")
                got = run_extract(lib, case, bufs, want_scan, with_recs, with_xs, n_rec, n_ops)
                check_extract(case, got, want, n_rec, n_ops, how)
                results[how] = got
        for k in ("pos", "flag", "tid", "cig_off", "cigar"):
            assert results["walk"][k].tobytes() == results["wave"][k].tobytes() == results["walk+xs"][k].tobytes() == results["wave+xs"][k].tobytes()
        assert results["walk+xs"]["xs"].tobytes() == results["wave+xs"]["xs"].tobytes()
        n_extracted += 1
    assert n_extracted > 0 or family in (8, 9)
    if family == 8:
        assert n_extracted > 0


@pytest.mark.parametrize("n,runs,cap", sc.bounds_cases())
def test_bounds(lib, n, runs, cap):
    tid, cig_off, want = sc.bounds_input(n, runs, 7 * n + runs)
    d_tid, d_cig_off = _dev(tid), _dev(cig_off)
    d_bounds = _out(16 * cap)
    d_n = torch.zeros(1 + 8, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert lib.spl_dev_launch_bam_bounds(_p(d_tid), _p(d_cig_off), ctypes.c_uint64(n), _p(d_bounds), _p(d_n), ctypes.c_uint32(cap), ctypes.c_void_p(0)) == 0
    torch.cuda.synchronize()
    counts = d_n.cpu().numpy()
    assert counts[0] == runs and not counts[1:].any()
    pairs = _host(d_bounds, 16 * cap, np.uint64, "bounds").reshape(cap, 2)       # (with cap + 1 runs too: nothing behind the cap-th pair)
    got = {(int(a), int(b)) for a, b in pairs[:min(runs, cap)]}
    assert len(got) == min(runs, cap)
    if runs <= cap:
        assert got == want
        assert pairs[runs:].tobytes() == bytes([FILL]) * (16 * (cap - runs))
    else:
        assert got < want


@pytest.fixture(scope="module")
def ctx():
    native.build()
    with native.Context(0) as c:
        yield c


SETTINGS = {"production": {}, "window2": {"SPL_INFLATE_WINDOW_BLOCKS": "2"}, "window3": {"SPL_INFLATE_WINDOW_BLOCKS": "3"}, "walk": {"SPL_EXTRACT_WALK": "1"}}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("family", (1, 2, 3, 4, 5, 6, 11))
def test_through_the_decoder(ctx, tmp_path, monkeypatch, family, setting):
    """The cases as files, one BGZF block per table entry: what the reference's rule lets through must be TAKEN -- decode_on_device
    True, no reason to decline -- and either way the arrays are what was written.  (A file the rule says must be taken and the
    device declines is a finding, not an expectation to relax.)"""
    for k, v in SETTINGS[setting].items():
        monkeypatch.setenv(k, v)
    n_taken = 0
    for k, case in enumerate(sc.cases(family)):
        if (case.tid_lo, case.tid_hi) != (0, case.n_ref + 1):       # (the decoder's window is all references: the same file as its neighbour)
            continue
        reason = sc.decline_reason(case, sc.reference(case)[0])
        path = str(tmp_path / ("f%d.bam" % k))
        write_file(case, path)
        for aux in ((False, True) if family == 11 else (False,)):
            dev = native.BamFile(path, threads=2, defer=True, min_mapq=case.filt[0], require_flags=case.filt[1], exclude_flags=case.filt[2], aux_strand=aux)
            took = dev.decode_on_device(ctx)
            assert took is (reason == ""), (case.name, dev.decline_reason(), reason)
            if setting == "production":
                assert dev.decline_reason() == reason, case.name
            n_kept = check_reads(dev, case, want_xs=aux)
            assert dev.n_records == len(case.offsets)
            if took:
                scan = sc.reference(case)[0]
                assert dev.filter_counts() == (int(scan["n_drop_flags"].sum()), int(scan["n_drop_mapq"].sum())) and n_kept == int(scan["n_placed"].sum())
            n_taken += took
            dev.close()
    assert n_taken > 0


def test_the_first_decoy_is_declined_and_the_host_is_right(ctx, tmp_path):
    case = next(c for c in sc.cases(10) if c.name == "decoy/four/cut")
    assert sc.decline_reason(case, sc.reference(case)[0]) == "a guessed record boundary did not hold"
    path = str(tmp_path / "decoy.bam")
    write_file(case, path)
    dev = native.BamFile(path, threads=2, defer=True)
    assert dev.decode_on_device(ctx) is False
    assert dev.decline_reason() == "a guessed record boundary did not hold"
    check_reads(dev, case)
    assert dev.n_records == len(case.offsets)
    dev.close()
