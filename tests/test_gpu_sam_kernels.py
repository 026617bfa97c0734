"""The kernels of spl_sam.hip on the texts of samcases.py, launched one by one through ctypes on torch buffers with guard bytes
behind every output: the line starts (count and fill), what the scan says of every line, the flagstat rows, the first declined
line and its reason, every extracted array and the order flag -- all against the Python restatement of the rule.  The bytes
behind a text are newlines here: none of them may count."""
import ctypes

import numpy as np
import pytest

import samcases as S
from spliser_amd import native

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD, FILL = 256, 0xA5
R0, O0 = 3, 5        # where the window's records and ops go in the output arrays: not at their beginning
NONE = (1 << 64) - 1
COUNTS = np.dtype([("first_bad", "<u8"), ("n_drop_flags", "<u4"), ("n_drop_mapq", "<u4"), ("unordered", "<u4"), ("overflow", "<u4")])
CASES = S.accepted_cases() + [c for c, _, reason in S.decline_cases() if reason != S.R["LONG_LINE"]]


class Names(ctypes.Structure):
    _fields_ = [("slots", ctypes.c_void_p), ("name_off", ctypes.c_void_p), ("blob", ctypes.c_void_p), ("n_slots", ctypes.c_uint32), ("n", ctypes.c_int32)]


@pytest.fixture(scope="module")
def lib():
    native.build()
    L = native.lib()
    L.spl_sam_chunks.restype = ctypes.c_uint32
    return L


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


def fnv1a(name):
    h = 2166136261
    for b in name:
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def name_table(ref_names):
    """The look-up table as the header says it is made (open addressing, linear probing from the FNV-1a hash), on the device."""
    n_slots = 4
    while n_slots < 2 * len(ref_names):
        n_slots *= 2
    slots = np.zeros(n_slots, np.uint32)
    blob = b"".join(n.encode("ascii") for n in ref_names)
    off = np.concatenate(([0], np.cumsum([len(n) for n in ref_names]))).astype(np.uint32)
    for t, n in enumerate(ref_names):
        s = fnv1a(n.encode("ascii")) & (n_slots - 1)
        while slots[s]:
            s = (s + 1) & (n_slots - 1)
        slots[s] = t + 1
    bufs = (_dev(slots), _dev(off), _dev(np.frombuffer(blob or b"\x00", np.uint8)))
    return Names(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), n_slots, len(ref_names)), bufs


def window(text, lo, hi):
    """-> (device buffer holding bytes [lo & ~15, hi) and newlines up to the pad's end, the pointer the kernels index with file offsets)."""
    base, hi16 = lo & ~15, (hi + 15) & ~15
    raw = text[base:hi] + b"\n" * (hi16 - hi + S.PAD)
    buf = _dev(np.frombuffer(raw, np.uint8))
    return buf, ctypes.c_void_p(buf.data_ptr() - base)


def run_line_starts(lib, text, lo, hi, want):
    base = lo & ~15
    buf, ptr = window(text, lo, hi)
    n_chunks = lib.spl_sam_chunks(ctypes.c_uint64(lo), ctypes.c_uint64(hi))
    assert n_chunks == (-(-(hi - base) // S.CHUNK) if hi > lo else 0)
    want = np.asarray(want, np.int64)
    per_chunk = np.bincount((want - base) // S.CHUNK, minlength=n_chunks).astype(np.uint32)
    d_count = _out(4 * n_chunks)
    assert lib.spl_dev_launch_sam_line_count(ptr, ctypes.c_uint64(lo), ctypes.c_uint64(hi), _p(d_count), ctypes.c_void_p(0)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_host(d_count, 4 * n_chunks, np.uint32, "chunk counts"), per_chunk)
    d_end, d_start = _dev(np.cumsum(per_chunk).astype(np.uint32)), _out(4 * len(want))
    assert lib.spl_dev_launch_sam_line_fill(ptr, ctypes.c_uint64(lo), ctypes.c_uint64(hi), _p(d_end), _p(d_start), ctypes.c_void_p(0)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_host(d_start, 4 * len(want), np.uint32, "line starts"), (want - base).astype(np.uint32))
    return buf, ptr


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_kernels_against_the_restatement(lib, case):
    ref, text = S.reference(case), case.text()
    lo, hi, base = case.begin, len(text), case.begin & ~15
    n = len(ref.starts)
    buf, ptr = run_line_starts(lib, text, lo, hi, ref.starts)
    if n == 0:
        return
    names, keep_alive = name_table(case.ref_names)
    d_start = _dev((np.asarray(ref.starts, np.int64) - base).astype(np.uint32))
    rows = (n + 63) // 64
    d_kept, d_nops, d_ltid, d_fstat = _out(4 * n), _out(4 * n), _out(4 * n), _out(64 * rows)
    counts = np.zeros(1, COUNTS)
    counts["first_bad"] = NONE
    d_counts = _dev(counts)
    q, f, F = case.filt
    assert lib.spl_dev_launch_sam_scan(ptr, ctypes.c_uint64(base), _p(d_start), ctypes.c_uint32(n), ctypes.c_uint64(ref.last_end), ctypes.byref(names), ctypes.c_uint32(q),
                                       ctypes.c_uint32(f), ctypes.c_uint32(F), ctypes.c_int(1), _p(d_kept), _p(d_nops), _p(d_ltid), _p(d_fstat), _p(d_counts), ctypes.c_void_p(0)) == 0
    torch.cuda.synchronize()
    kept, nops, ltid = (_host(d, 4 * n, dt, what) for d, dt, what in ((d_kept, np.uint32, "kept"), (d_nops, np.uint32, "n_ops"), (d_ltid, np.int32, "line_tid")))
    want_ops = [len(g["ops"]) if k else 0 for k, (_, g) in zip(ref.kept_mask, ref.lines)]
    assert kept.tolist() == ref.kept_mask and nops.tolist() == want_ops
    assert ltid.tolist() == [-1 if reason else g["tid"] for reason, g in ref.lines]
    got = d_counts.cpu().numpy().view(COUNTS)[0]
    bad = [(k << 8 | reason) for k, (reason, _) in enumerate(ref.lines) if reason]
    assert int(got["first_bad"]) == (bad[0] if bad else NONE)
    assert [int(got["n_drop_flags"]), int(got["n_drop_mapq"])] == ref.dropped and int(got["overflow"]) == 0
    fstat = _host(d_fstat, 64 * rows, np.uint32, "flagstat rows").reshape(rows, 16).astype(np.int64)
    assert np.array_equal(np.stack([(fstat & 0xFFFF).sum(axis=0), (fstat >> 16).sum(axis=0)], axis=1), ref.flagstat)
    if ref.decline is not None:
        return
    # ---- the extraction, its records behind R0 others and its ops behind O0
    n_rec, n_ops = len(ref.pos), len(ref.cigar)
    d_kend, d_oend = _dev(np.cumsum(kept).astype(np.uint32)), _dev(np.cumsum(nops).astype(np.uint32))
    outs = dict(pos=_out(4 * (R0 + n_rec)), flag=_out(2 * (R0 + n_rec)), tid=_out(4 * (R0 + n_rec)), cig_off=_out(4 * (R0 + n_rec + 1)), cigar=_out(4 * (O0 + n_ops)), xs=_out(R0 + n_rec))
    d_max = torch.zeros(len(case.ref_names) + 8, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()

    def extract(cap_rec, cap_ops):
        rc = lib.spl_dev_launch_sam_extract(ptr, ctypes.c_uint64(base), _p(d_start), ctypes.c_uint32(n), ctypes.c_uint64(ref.last_end), ctypes.byref(names), ctypes.c_uint32(q),
                                            ctypes.c_uint32(f), ctypes.c_uint32(F), _p(d_kend), _p(d_oend), _p(d_ltid), ctypes.c_uint64(R0), ctypes.c_uint64(O0),
                                            ctypes.c_uint64(cap_rec), ctypes.c_uint64(cap_ops), _p(outs["pos"]), _p(outs["flag"]), _p(outs["tid"]), _p(outs["cig_off"]),
                                            _p(outs["cigar"]), _p(outs["xs"]), _p(d_max), _p(d_counts), ctypes.c_void_p(0))
        assert rc == 0
        torch.cuda.synchronize()
    extract(R0 + n_rec, O0 + n_ops)
    assert int(d_counts.cpu().numpy().view(COUNTS)[0]["overflow"]) == 0
    want = dict(pos=ref.pos, flag=ref.flag, tid=ref.tid, cig_off=ref.cig_off[1:] + np.uint32(O0), cigar=ref.cigar, xs=ref.xs)
    sizes = dict(pos=4, flag=2, tid=4, cig_off=4, cigar=4, xs=1)
    for k, dt in (("pos", np.int32), ("flag", np.uint16), ("tid", np.int32), ("cig_off", np.uint32), ("cigar", np.uint32), ("xs", np.uint8)):
        lead = (O0 if k == "cigar" else R0 + 1 if k == "cig_off" else R0)
        a = _host(outs[k], sizes[k] * (lead + len(want[k])), dt, k)
        assert a[:lead].tobytes() == bytes([FILL]) * (lead * sizes[k]), "%s: %s written in front of the first record" % (case.name, k)
        assert np.array_equal(a[lead:], want[k]), "%s: %s" % (case.name, k)
    assert [int(x) for x in d_max.cpu().numpy()[:len(case.ref_names)]] == ref.max_end and not d_max.cpu().numpy()[len(case.ref_names):].any()
    # ---- whether reference ids or POS go down
    d_tid, d_pos = _dev(ref.tid), _dev(ref.pos)
    assert lib.spl_dev_launch_sam_order(_p(d_tid), _p(d_pos), ctypes.c_uint64(0), ctypes.c_uint64(n_rec), _p(d_counts), ctypes.c_void_p(0)) == 0
    torch.cuda.synchronize()
    assert bool(d_counts.cpu().numpy().view(COUNTS)[0]["unordered"]) == ref.unordered
    del keep_alive, buf


def test_line_starts_of_a_window_inside_the_text(lib):
    """[lo, hi) in the middle of the large case, lo neither a multiple of 16 nor of a chunk, newlines in front of lo and behind hi."""
    case = S.large_case()
    ref, text = S.reference(case), case.text()
    for a, b in ((100, 2500), (1, 2), (2999, 3400), (5, len(ref.starts) - 1)):
        lo, hi = ref.starts[a], ref.starts[b]
        run_line_starts(lib, text, lo, hi, ref.starts[a:b])


def test_extraction_told_of_less_room_writes_nothing_beyond_it(lib):
    case = S.large_case()
    ref, text = S.reference(case), case.text()
    base, n = case.begin & ~15, len(ref.starts)
    buf, ptr = window(text, case.begin, len(text))
    names, keep_alive = name_table(case.ref_names)
    d_start = _dev((np.asarray(ref.starts, np.int64) - base).astype(np.uint32))
    kept = np.asarray(ref.kept_mask, np.uint32)
    nops = np.array([len(g["ops"]) if k else 0 for k, (_, g) in zip(ref.kept_mask, ref.lines)], np.uint32)
    d_kend, d_oend, d_ltid = _dev(np.cumsum(kept).astype(np.uint32)), _dev(np.cumsum(nops).astype(np.uint32)), _dev(np.array([g["tid"] for _, g in ref.lines], np.int32))
    n_rec, n_ops = len(ref.pos) - 100, len(ref.cigar) - 150        # (the arrays are that short, and the kernel is told so)
    outs = [_out(4 * n_rec), _out(2 * n_rec), _out(4 * n_rec), _out(4 * (n_rec + 1)), _out(4 * n_ops), _out(n_rec)]
    d_max = torch.zeros(len(case.ref_names), dtype=torch.int64, device="cuda:0")
    d_counts = _dev(np.zeros(1, COUNTS))
    rc = lib.spl_dev_launch_sam_extract(ptr, ctypes.c_uint64(base), _p(d_start), ctypes.c_uint32(n), ctypes.c_uint64(ref.last_end), ctypes.byref(names), ctypes.c_uint32(0),
                                        ctypes.c_uint32(0), ctypes.c_uint32(0), _p(d_kend), _p(d_oend), _p(d_ltid), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(n_rec),
                                        ctypes.c_uint64(n_ops), *[_p(o) for o in outs], _p(d_max), _p(d_counts), ctypes.c_void_p(0))
    assert rc == 0
    torch.cuda.synchronize()
    assert int(d_counts.cpu().numpy().view(COUNTS)[0]["overflow"]) == 1
    for o, size, what in zip(outs, (4 * n_rec, 2 * n_rec, 4 * n_rec, 4 * (n_rec + 1), 4 * n_ops, n_rec), ("pos", "flag", "tid", "cig_off", "cigar", "xs")):
        _host(o, size, np.uint8, what)
    del keep_alive, buf
