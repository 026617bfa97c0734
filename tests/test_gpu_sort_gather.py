"""The gather side of ``--anyOrder`` and the device-wide scan, launched one by one through ctypes on torch buffers with guard bytes
behind every output, at the sizes where their loops take a second trip (tests/gathercases.py; tests/test_gathercases_host.py proves
where each size lies): ``spl_dev_launch_sort_scan`` against numpy's ``cumsum`` in 64 bits, ``make_keys`` against ``tid << 32 | pos``,
``gather`` (both instantiations) and ``cigar`` against fancy indexing, and one ``--anyOrder`` decode of 2 100 000 records -- above both
thresholds, so every kernel of RecordSort::run leaves its first trip -- against numpy's stable sort of what was written.  Everything
is exact.  The reference has no counterpart: it reads a file that ``samtools sort`` has put in order (SpliSER_v0_1_8.py:422)."""
import ctypes
import time

import numpy as np
import pytest

import gathercases as G
import ordercases as O
from spliser_amd import native
from test_gpu_sam_kernels import FILL, GUARD, _dev, _host, _out, _p

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

INVALID_VALUE = 1      # (hipErrorInvalidValue)
NULL = ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def lib():
    native.build()
    L = native.lib()
    L.spl_dev_sort_work_bytes.restype = ctypes.c_size_t
    L.spl_dev_sort_parts.restype = ctypes.c_uint32
    return L


def _inout(a, lead=0):
    """A guarded buffer that begins with ``lead`` bytes of the fill and then holds ``a`` -> (buffer, bytes of a)."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = _out(lead + len(raw))
    if len(raw):
        t[lead:lead + len(raw)] = torch.from_numpy(raw.copy()).to("cuda:0")
    return t, len(raw)


def _at(t, byte_offset):
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


def _untouched(t, what):
    assert bool((t == FILL).all().item()), what + " was written"


def run_scan(lib, v, lead=0):
    """The scan of ``v`` in place, ``lead`` bytes into its allocation -> the sums; the bytes in front of v, behind it and behind the
    work buffer must be as they were."""
    n = len(v)
    assert lib.spl_dev_sort_parts(ctypes.c_uint64(n)) == G.plan(n)[2]
    n_work = lib.spl_dev_sort_work_bytes(ctypes.c_uint64(n))
    assert n_work >= 4 * (G.plan(n)[2] + 1)
    d_v, n_bytes = _inout(v, lead)
    d_work = _out(n_work)
    assert lib.spl_dev_launch_sort_scan(_at(d_v, lead), ctypes.c_uint64(n), _p(d_work), NULL) == 0
    torch.cuda.synchronize()
    _host(d_work, n_work, np.uint8, "the scan's work buffer")
    raw = _host(d_v, lead + n_bytes, np.uint8, "the scanned values")
    assert raw[:lead].tobytes() == bytes([FILL]) * lead, "written in front of the scanned values"
    return raw[lead:].view(np.uint32)


# ---- the scan -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", G.SCAN_SIZES)
def test_the_scan_against_cumsum(lib, n):
    for kind in G.SCAN_KINDS:
        v = G.scan_values(kind, n)
        got, want = run_scan(lib, v), G.scan_expected(v)
        assert np.array_equal(got, want), (n, kind, np.flatnonzero(got != want)[:4].tolist())


def test_the_scan_up_to_the_largest_32_bit_total(lib):
    """S1 + 1 values (two tiles a part) of 2047, the last one larger: the total is exactly 2^32 - 1, and no sum on the way wraps."""
    v = G.scan_values("full", G.S1 + 1)
    got, want = run_scan(lib, v), G.scan_expected(v)
    assert int(want[-1]) == 0xFFFFFFFF
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:4].tolist()


@pytest.mark.parametrize("n", [G.TILE + 1, G.S1 + 1])
def test_the_scan_of_values_four_bytes_into_an_allocation(lib, n):
    """As RecordSort::run calls it: on ``cigoff2 + 1``, whose address is 4 modulo 16."""
    v = G.scan_values("mixed", n)
    got, want = run_scan(lib, v, lead=4), G.scan_expected(v)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:4].tolist()


def test_the_scan_without_a_work_buffer_launches_nothing(lib):
    d_v, n_bytes = _inout(G.scan_values("ones", 100))
    assert lib.spl_dev_launch_sort_scan(_p(d_v), ctypes.c_uint64(100), NULL, NULL) == INVALID_VALUE
    torch.cuda.synchronize()
    assert np.array_equal(_host(d_v, n_bytes, np.uint32, "the values"), np.ones(100, np.uint32))


# ---- make_keys ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", G.GATHER_SIZES)
def test_make_keys(lib, n):
    tid, pos = G.key_fields(n)
    d_tid, d_pos, d_keys = _dev(tid), _dev(pos), _out(8 * n)
    assert lib.spl_dev_launch_sort_make_keys(_p(d_tid), _p(d_pos), ctypes.c_uint64(n), _p(d_keys), NULL) == 0
    torch.cuda.synchronize()
    got, want = _host(d_keys, 8 * n, np.uint64, "keys"), G.keys_expected(tid, pos)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:4].tolist()


def test_make_keys_of_no_record_launches_nothing(lib):
    d_keys = _out(0)
    assert lib.spl_dev_launch_sort_make_keys(NULL, NULL, ctypes.c_uint64(0), _p(d_keys), NULL) == 0
    torch.cuda.synchronize()
    _untouched(d_keys, "keys")


# ---- gather, scan, cigar ------------------------------------------------------------------------------------------------------------

FIELDS = (("pos", 4, np.int32), ("flag", 2, np.uint16), ("xs", 1, np.uint8), ("tid", 4, np.int32))


def _gather_outputs(n):
    outs = {k: _out(size * n) for k, size, _ in FIELDS}
    outs["cig_off"] = _out(4 * (n + 1))
    return outs


def _launch_gather(lib, n, ins, outs, xs_in, xs_out):
    return lib.spl_dev_launch_sort_gather(_p(ins["perm"]), _p(ins["keys"]), ctypes.c_uint64(n), _p(ins["pos"]), _p(ins["flag"]), _p(ins["xs"]) if xs_in else NULL, _p(ins["cig_off"]),
                                          _p(outs["pos"]), _p(outs["flag"]), _p(outs["xs"]) if xs_out else NULL, _p(outs["tid"]), _p(outs["cig_off"]), NULL)


@pytest.mark.parametrize("n", G.GATHER_SIZES)
def test_gather_scan_and_cigar(lib, n):
    case = G.GatherCase(n)
    want = case.expected()
    ins = dict(perm=_dev(case.perm), keys=_dev(case.keys), pos=_dev(case.pos), flag=_dev(case.flag), xs=_dev(case.xs), cig_off=_dev(case.cig_off), cigar=_dev(case.cigar))
    n_ops = len(case.cigar)
    for with_xs in (True, False):
        outs = _gather_outputs(n)
        assert _launch_gather(lib, n, ins, outs, with_xs, with_xs) == 0
        torch.cuda.synchronize()
        for k, size, dt in FIELDS:
            if k == "xs" and not with_xs:
                _untouched(outs["xs"], "xs_out, with no strand bytes asked for,")
                continue
            got = _host(outs[k], size * n, dt, k)
            assert np.array_equal(got, want[k]), (n, with_xs, k, np.flatnonzero(got != want[k])[:4].tolist())
        got = _host(outs["cig_off"], 4 * (n + 1), np.uint32, "cig_off_out")
        assert np.array_equal(got, want["counts"]), (n, with_xs, "the op counts", np.flatnonzero(got != want["counts"])[:4].tolist())
        # the scan, as RecordSort::run calls it: on cig_off_out + 1
        n_work = lib.spl_dev_sort_work_bytes(ctypes.c_uint64(n))
        d_work = _out(n_work)
        assert lib.spl_dev_launch_sort_scan(_at(outs["cig_off"], 4), ctypes.c_uint64(n), _p(d_work), NULL) == 0
        torch.cuda.synchronize()
        _host(d_work, n_work, np.uint8, "the scan's work buffer")
        got = _host(outs["cig_off"], 4 * (n + 1), np.uint32, "cig_off_out")
        assert np.array_equal(got, want["cig_off"]), (n, with_xs, "cig_off", np.flatnonzero(got != want["cig_off"])[:4].tolist())
        d_cigar = _out(4 * n_ops)
        assert lib.spl_dev_launch_sort_cigar(_p(ins["perm"]), ctypes.c_uint64(n), _p(ins["cig_off"]), _p(ins["cigar"]), _p(outs["cig_off"]), _p(d_cigar), NULL) == 0
        torch.cuda.synchronize()
        got = _host(d_cigar, 4 * n_ops, np.uint32, "cigar_out")
        assert np.array_equal(got, want["cigar"]), (n, with_xs, "cigar", np.flatnonzero(got != want["cigar"])[:4].tolist())
    # the inputs are as they were
    for k, a in (("perm", case.perm), ("keys", case.keys), ("pos", case.pos), ("flag", case.flag), ("xs", case.xs), ("cig_off", case.cig_off), ("cigar", case.cigar)):
        assert ins[k].cpu().numpy().tobytes() == a.tobytes(), k


@pytest.mark.parametrize("xs_in, xs_out", [(True, False), (False, True)])
def test_gather_with_strand_bytes_on_one_side_only_launches_nothing(lib, xs_in, xs_out):
    n = 257
    case = G.GatherCase(n)
    ins = dict(perm=_dev(case.perm), keys=_dev(case.keys), pos=_dev(case.pos), flag=_dev(case.flag), xs=_dev(case.xs), cig_off=_dev(case.cig_off))
    outs = _gather_outputs(n)
    assert _launch_gather(lib, n, ins, outs, xs_in, xs_out) == INVALID_VALUE
    torch.cuda.synchronize()
    for k, t in outs.items():
        _untouched(t, k + "_out")


def test_gather_and_cigar_of_no_record_launch_nothing(lib):
    outs = _gather_outputs(0)
    d_cigar = _out(0)
    assert lib.spl_dev_launch_sort_gather(NULL, NULL, ctypes.c_uint64(0), NULL, NULL, NULL, NULL, _p(outs["pos"]), _p(outs["flag"]), _p(outs["xs"]), _p(outs["tid"]), _p(outs["cig_off"]), NULL) == 0
    assert lib.spl_dev_launch_sort_cigar(NULL, ctypes.c_uint64(0), NULL, NULL, _p(outs["cig_off"]), _p(d_cigar), NULL) == 0
    torch.cuda.synchronize()
    for k, t in list(outs.items()) + [("cigar", d_cigar)]:
        _untouched(t, k + "_out")


# ---- the whole chain, once, above both thresholds -----------------------------------------------------------------------------------

def test_any_order_decode_of_2_100_000_records(lib, tmp_path):
    """2 100 000 records of three references, interleaved, POS from 1..4096: make_keys, the passes, gather, scan and cigar all leave
    their first trip in one RecordSort::run (five trips of the gather's loops, two tiles a part).  Per reference the arrays are
    numpy's stable sort of what was written.  The file is written at level 0 (stored blocks: 0.7 s on a slow host where level 1
    took 1.5 s).  Measured on an MI355X: 0.40 s in all -- the file 0.19 s, decode and sort 0.06 s, the comparison 0.15 s."""
    t0 = time.perf_counter()
    n = G.DECODE_RECORDS
    tid, pos, flag, op = G.decode_fields(n)
    path = str(tmp_path / "large.bam")
    # ordercases.write_bam's framing -- header, BGZF blocks, the end-of-file block -- around records made as one array: the file
    # without records first, then the records' blocks in front of its end-of-file block
    O.write_bam(path, G.DECODE_REFS, [1 << 20] * 3, [], so="unsorted", level=0)
    with open(path, "r+b") as fh:
        fh.seek(-len(O.EOF_BLOCK), 2)
        assert fh.read() == O.EOF_BLOCK
        fh.seek(-len(O.EOF_BLOCK), 2)
        fh.write(O.bgzf(G.bam_records(tid, pos, flag, op), level=0))
        fh.write(O.EOF_BLOCK)
    t1 = time.perf_counter()
    with native.Context(0) as ctx:
        bam = native.BamFile(path, threads=3, defer=True, any_order=True)
        bam.decode_on_device(ctx)
        assert bam.on_device is True, bam.decline_reason()
        assert bam.wait_all() is True
        assert bam.decline_reason() == ""
        assert bam.any_order_sorted() == (n, True)
        t2 = time.perf_counter()
        for t, name in enumerate(G.DECODE_REFS):
            w_pos, w_flag, w_off, w_cigar = G.decode_expected(tid, pos, flag, op, t)
            got = bam.reads(name)
            assert got.n == len(w_pos), name
            assert np.array_equal(got.pos, w_pos), (name, "pos")
            assert np.array_equal(got.flag, w_flag), (name, "flag")
            assert np.array_equal(got.cig_off, w_off), (name, "cig_off")
            assert np.array_equal(got.cigar, w_cigar), (name, "cigar")
            del got
        bam.close()
    t3 = time.perf_counter()
    print("2 100 000 records: file written in %.2f s, decoded and sorted in %.2f s, compared in %.2f s" % (t1 - t0, t2 - t1, t3 - t2))
