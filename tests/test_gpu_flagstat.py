"""The flagstat counters on the GPU (``spl_bam_set_flagstat``): the record scan's counting instantiation and the reduce kernel on
hand-built streams against the restatement of ``flagstatcases`` -- word for word per block, then added up --, the device decode of
files cut inside records with windows of a few blocks and in shares (a block scanned twice counts once, a record belongs to the
share its first byte lies in), the width of the counters, and the commands."""
import ctypes
import os

import numpy as np
import pytest

import filtercases as F
import flagstatcases as fc
import scancases as sc
from spliser_amd import cli, flagstat, native

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD, FILL = 256, 0xA5


@pytest.fixture(scope="module")
def lib():
    native.build()
    return native.lib()


@pytest.fixture(scope="module")
def ctx():
    with native.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def mixed():
    return fc.mix(seed=5, n=700, body=120)


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


def reduce_on_device(lib, d_fstat, n_blocks, sums0=None):
    d_sums = torch.zeros(32, dtype=torch.int64, device="cuda:0") if sums0 is None else sums0
    assert lib.spl_dev_launch_bam_flagstat_reduce(_p(d_fstat), ctypes.c_uint32(n_blocks), _p(d_sums), ctypes.c_void_p(0)) == 0
    torch.cuda.synchronize()
    return d_sums.cpu().numpy().reshape(16, 2)


def scan_and_reduce(lib, b, lens, filt=(0, 0, 0)):
    """The counting scan over the whole stream of ``b`` tiled by ``lens`` -> (fstat as uint32 (blocks, 16), the reduced sums (16, 2))."""
    blocks = np.zeros(len(lens), sc.ZBLOCK)
    blocks["out_len"] = lens
    blocks["out"] = np.concatenate(([0], np.cumsum(lens)[:-1]))
    n = len(lens)
    d_stream, d_blocks = _dev(np.frombuffer(b.stream + b"\xee" * sc.PAD, np.uint8)), _dev(blocks)
    d_scan, d_fstat = _out(n * sc.BSCAN.itemsize), _out(n * 64)
    rc = lib.spl_dev_launch_bam_scan2(_p(d_stream), ctypes.c_uint64(len(b.stream)), ctypes.c_uint64(len(b.header)), ctypes.c_int32(b.n_ref), ctypes.c_int32(0),
                                      ctypes.c_int32(b.n_ref + 1), _p(d_blocks), ctypes.c_uint32(n), _p(d_scan), ctypes.c_int(0), ctypes.c_void_p(0),
                                      ctypes.c_uint32(filt[0]), ctypes.c_uint32(filt[1]), ctypes.c_uint32(filt[2]), ctypes.c_void_p(0), _p(d_fstat))
    assert rc == 0
    torch.cuda.synchronize()
    scan = _host(d_scan, n * sc.BSCAN.itemsize, sc.BSCAN, "scan")
    assert not np.any(scan["flags"]), scan["flags"]
    fstat = _host(d_fstat, n * 64, np.uint32, "fstat").reshape(n, 16).copy()
    return fstat, reduce_on_device(lib, d_fstat, n), scan


def _decode(path, ctx, filt=(0, 0, 0), devices=None):
    bam = native.BamFile(path, threads=2, defer=True, min_mapq=filt[0], require_flags=filt[1], exclude_flags=filt[2], flagstat=True)
    if devices is None:
        assert bam.decode_on_device(ctx) is True, bam.decline_reason()
    else:
        assert len(bam.decode_on_devices_async(list(devices))) == len(devices)
        assert bam.join_decoders() is True, bam.decline_reason()
    return bam


def _host_counts(path, filt=(0, 0, 0), threads=2):
    bam = native.BamFile(path, threads=threads, min_mapq=filt[0], require_flags=filt[1], exclude_flags=filt[2], flagstat=True)
    try:
        return bam.flagstat()
    finally:
        bam.close()


# ---- 1. scan + reduce on the smallest shapes ---------------------------------------------------------------------------------
def test_smallest_shapes(lib):
    one = fc.Built(2, [fc._rec(0, 7, 0x1 | 0x40 | 0x200, 5, 1)], [(0x1 | 0x40 | 0x200, 0, 1, 5)])
    fstat, sums, scan = scan_and_reduce(lib, one, [len(one.stream)])
    assert np.array_equal(fstat, one.want_packed([len(one.stream)])) and np.array_equal(sums, one.want())
    assert sums[0].tolist() == [0, 1] and sums[15].tolist() == [0, 1] and int(scan["n_all"][0]) == 1
    none = fc.Built(2, [], [])
    fstat, sums, scan = scan_and_reduce(lib, none, [len(none.stream)])
    assert not fstat.any() and not sums.any() and int(scan["n_all"][0]) == 0
    # blocks of BAM header bytes only, and an empty block where the header ends: zeros, written (not the fill)
    head = fc.Built(2, [fc._rec(1, 3, 0, 60, -1)], [(0, 1, -1, 60)], text_len=300)
    H = len(head.header)
    lens = [100, H - 100, 0, len(head.stream) - H]
    fstat, sums, _ = scan_and_reduce(lib, head, lens)
    assert not fstat[:3].any() and np.array_equal(fstat, head.want_packed(lens)) and np.array_equal(sums, head.want())
    # four records that between them are in every category, QC-passed, and the same four QC-failed.  (Once each is as few as the
    # table allows: a singleton is primary, mapped and paired as the record with its mate elsewhere is.)
    rows = [(0x1 | 0x2 | 0x40 | 0x80 | 0x400, 0, 1, 5), (0x100 | 0x4, 0, -1, 0), (0x800 | 0x4, 0, -1, 0), (0x1 | 0x8, 0, 0, 0)]
    rows = rows + [(f | 0x200, t, n, q) for f, t, n, q in rows]
    once = fc.Built(2, [fc._rec(t, 5 + k, f, q, n) for k, (f, t, n, q) in enumerate(rows)], rows)
    want = once.want()
    assert np.array_equal(want[[2, 3, 4, 5, 9, 10, 11, 12, 13, 14, 15]], np.ones((11, 2), np.int64)) and want[0].tolist() == [4, 4] and want.min() == 1, want.T
    fstat, sums, _ = scan_and_reduce(lib, once, [len(once.stream)])
    assert np.array_equal(sums, want), (sums.T, want.T)
    assert np.array_equal(fstat, once.want_packed([len(once.stream)]))


def test_scan_per_block_against_the_restatement(lib, mixed):
    """Records of a few hundred bytes over blocks of 61, 700 and 4096 bytes: a record counts in the block its first byte lies in, once."""
    for L in (61, 700, 4096):
        lens = mixed.tiles(L)
        fstat, sums, scan = scan_and_reduce(lib, mixed, lens)
        want = mixed.want_packed(lens)
        bad = np.flatnonzero((fstat != want).any(axis=1))
        assert len(bad) == 0, (L, bad[0], fstat[bad[0]], want[bad[0]])
        assert np.array_equal(sums, mixed.want())
        assert int(scan["n_all"].sum()) == mixed.n_records == int(sums[0].sum())
        cuts = mixed.cut_points(lens)
        assert sum(mixed.straddled(int(c)) for c in cuts) > len(cuts) // 2       # (most cuts fall inside a record)
    for filt in (F.FILTER_A, F.FILTER_B):
        lens = mixed.tiles(700)
        fstat, sums, scan = scan_and_reduce(lib, mixed, lens, filt)
        assert np.array_equal(fstat, mixed.want_packed(lens, filt)) and np.array_equal(sums, mixed.want(filt))
        assert int(scan["n_all"].sum()) == mixed.n_records          # (the scan's own counters: untouched by the counting)


# ---- 3. counter width, the reduce kernel's shapes -------------------------------------------------------------------------------
@pytest.mark.parametrize("n_blocks", [1, 3, 4, 5, 63, 64, 65, 257])
def test_reduce_kernel_shapes(lib, n_blocks):
    """Partial groups of four blocks a wave, more than one workgroup (sixteen blocks each), both halves at their largest."""
    rng = np.random.default_rng(n_blocks)
    words = rng.integers(0, 1 << 32, (n_blocks, 16), dtype=np.uint64).astype(np.uint32)
    words[0] = 0xFFFFFFFF
    words[-1, ::2] = 0xFFFF0000
    d = _out(n_blocks * 64)
    d[:n_blocks * 64] = _dev(words)
    want = np.stack([(words & 0xFFFF).astype(np.int64).sum(axis=0), (words >> 16).astype(np.int64).sum(axis=0)], axis=1)
    got = reduce_on_device(lib, d, n_blocks)
    assert np.array_equal(got, want)
    # the sums only grow: a second launch over the first three blocks adds those
    start = torch.from_numpy(got.reshape(-1).copy()).to("cuda:0")
    k = min(3, n_blocks)
    again = reduce_on_device(lib, d, k, start)
    want2 = want + np.stack([(words[:k] & 0xFFFF).astype(np.int64).sum(axis=0), (words[:k] >> 16).astype(np.int64).sum(axis=0)], axis=1)
    assert np.array_equal(again, want2)
    _host(d, n_blocks * 64, np.uint32, "fstat")


def test_counter_width(lib, ctx, tmp_path):
    """Blocks of nothing but 37-byte QC-failed records: a block's high halves reach the most records that can begin in one with the low
    halves at zero; 41 such blocks take the reduced sums past 65 535."""
    b, lens = fc.full_blocks(41)
    assert len(lens) >= 42 and lens[1] == 65536
    fstat, sums, scan = scan_and_reduce(lib, b, lens)
    owner = np.bincount(b.block_of_record(lens), minlength=len(lens))
    assert owner[1] == 1772 and owner.max() <= sc.REC_CAP
    assert np.array_equal(fstat[:, 0] >> 16, owner) and not (fstat & 0xFFFF).any()
    assert np.array_equal(fstat, b.want_packed(lens))
    want = b.want()
    assert want[0, 1] == b.n_records > 65535 and want[15, 1] == b.n_records and not want[:, 0].any()
    assert np.array_equal(sums, want)
    # ... and as a file through the device decode, whole and in two shares
    path = b.write(str(tmp_path / "full.bam"), lens)
    for devices in (None, (0, 0)):
        bam = _decode(path, ctx, devices=devices)
        assert np.array_equal(bam.flagstat(), want) and bam.n_records == b.n_records
        bam.close()


# ---- 2. blocks and windows ------------------------------------------------------------------------------------------------------
def test_windows_count_a_block_once(ctx, mixed, tmp_path, monkeypatch):
    lens = mixed.tiles(3000)
    assert len(lens) > 30
    path = mixed.write(str(tmp_path / "w.bam"), lens)
    edges = np.concatenate(([0], np.cumsum(lens)))
    want = mixed.want()
    seen = []
    for window in (None, "2", "3", "7"):
        if window is None:
            monkeypatch.delenv("SPL_INFLATE_WINDOW_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("SPL_INFLATE_WINDOW_BLOCKS", window)
            w = int(window)
            crossed = [k for k in range(w, len(lens), w) if mixed.straddled(int(edges[k]))]
            assert crossed, "no record crosses a window edge"       # (the block it begins in waits for the next window: scanned twice)
        bam = _decode(path, ctx)
        got = bam.flagstat()
        assert np.array_equal(got, want), (window, got.T, want.T)
        assert bam.n_records == mixed.n_records == int(got[0].sum())
        seen.append(got)
        bam.close()
    assert all(np.array_equal(seen[0], s) for s in seen)
    monkeypatch.setenv("SPL_INFLATE_WINDOW_BLOCKS", "3")
    monkeypatch.setenv("SPL_EXTRACT_WALK", "1")
    bam = _decode(path, ctx, F.FILTER_B)
    assert np.array_equal(bam.flagstat(), mixed.want(F.FILTER_B))
    bam.close()


# ---- 4. shares --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_shares_add_up(ctx, mixed, tmp_path, devices, monkeypatch):
    lens = mixed.tiles(2500)
    path = mixed.write(str(tmp_path / "s.bam"), lens)
    for filt in ((0, 0, 0), F.FILTER_A):
        bam = _decode(path, ctx, filt, devices)
        infos = [bam.share_info(k) for k in range(len(devices))]
        edges = set(np.cumsum(lens).tolist())
        assert all(int(i["u_lo"]) in set(mixed.offsets.tolist()) for i in infos[1:])
        assert any(int(i["u_lo"]) not in edges for i in infos[1:]), "every share begins with a block's first byte: no cut fell inside a record"
        got = bam.flagstat()
        assert np.array_equal(got, mixed.want(filt)), (filt, got.T)
        assert bam.n_records == mixed.n_records
        if filt == (0, 0, 0):
            assert int(got[0].sum()) == mixed.n_records       # (every record is one share's, none is two shares')
        bam.close()
    monkeypatch.setenv("SPL_INFLATE_WINDOW_BLOCKS", "3")
    bam = _decode(path, ctx, (0, 0, 0), devices)
    assert np.array_equal(bam.flagstat(), mixed.want())
    bam.close()


# ---- 5. device == host decoder == restatement on the golden read sets, rebuilt with mates ------------------------------------------
@pytest.mark.parametrize("case,seed", [("junctions_u", 11), ("random_a", 12), ("combine_a/sample0", 13)])
def test_device_host_and_restatement_agree(ctx, tmp_path, case, seed, monkeypatch):
    b = fc.with_mates(case, seed)
    lens = b.tiles(9000)
    path = b.write(str(tmp_path / "g.bam"), lens)
    for filt in ((0, 0, 0), F.FILTER_A):
        want = b.want(filt)
        assert want[14, 0] > 0 and want[13, 0] > 0 and (want[3].sum() > 0 or filt[2] & 0x800)
        host = _host_counts(path, filt)
        assert np.array_equal(host, want), (filt, host.T, want.T)
        for walk in (False, True):
            if walk:
                monkeypatch.setenv("SPL_EXTRACT_WALK", "1")
            else:
                monkeypatch.delenv("SPL_EXTRACT_WALK", raising=False)
            bam = _decode(path, ctx, filt)
            got = bam.flagstat()
            assert np.array_equal(got, want), (filt, walk, got.T, want.T)
            bam.close()
    monkeypatch.delenv("SPL_EXTRACT_WALK", raising=False)


def test_off_means_unchanged(ctx, mixed, tmp_path):
    """The same file with and without the counters: the same reads, the same counters of the filter; and no counters to ask for."""
    path = mixed.write(str(tmp_path / "o.bam"), mixed.tiles(3000))
    on = _decode(path, ctx, F.FILTER_B)
    off = native.BamFile(path, threads=2, defer=True, min_mapq=F.FILTER_B[0], require_flags=F.FILTER_B[1], exclude_flags=F.FILTER_B[2])
    assert off.decode_on_device(ctx) is True
    for t in range(mixed.n_ref):
        F.same_reads(on.reads("c%d" % t), off.reads("c%d" % t), "c%d" % t)
    assert on.filter_counts() == off.filter_counts() and on.n_records == off.n_records
    with pytest.raises(native.SpliserNativeError):
        off.flagstat()
    with pytest.raises(native.SpliserNativeError):
        on.set_flagstat(False)
    on.close()
    off.close()


# ---- 6. the commands --------------------------------------------------------------------------------------------------------------
def test_commands(tmp_path, capsys):
    c = F.Case("junctions_u", 11, F.FILTER_A, repeat=2)
    x, _ = c.write(str(tmp_path / "p"), with_seq=True)
    bed = os.path.join(c.dir, "junctions.bed")
    out = lambda tag: str(tmp_path / tag)      # noqa: E731
    read = lambda path: open(path).read()      # noqa: E731
    flag = np.concatenate([rs.flag for _, rs in c.x])
    tid = np.concatenate([np.full(rs.n, k) for k, (_, rs) in enumerate(c.x)])
    for tag, filt, argv in (("all", (0, 0, 0), []), ("a", F.FILTER_A, ["--minMapQ", "255", "--excludeFlags", "0x900"])):
        w = fc.restate_filtered(flag, tid, np.full(len(flag), -1), np.concatenate(c.mapq), filt)
        assert cli.main(["flagstat", "-B", x, "-o", out(tag + ".host.txt"), "--hostDecode"] + argv) == 0
        want = read(out(tag + ".host.txt"))
        assert want == "\n".join(flagstat.format_lines(w)) + "\n"
        assert cli.main(["flagstat", "-B", x, "-o", out(tag + ".dev.txt")] + argv) == 0
        assert cli.main(["flagstat", "-B", x, "-o", out(tag + ".shares.txt"), "--devices", "0,0"] + argv) == 0
        assert read(out(tag + ".dev.txt")) == read(out(tag + ".shares.txt")) == want
        modes = (("b", ["-b", bed]), ("nb", ["--minAnchor", "1", "--minIntron", "1", "--maxIntron", "0"]), ("host", ["-b", bed, "--hostDecode"]),
                 ("keep", ["-b", bed, "--keepReads"]), ("gpus", ["-b", bed, "--devices", "0,0"]), ("chrom", ["-b", bed, "-c", c.names[0]]))
        for mode, extra in modes if tag == "all" else modes[:1]:
            capsys.readouterr()
            assert cli.main(["process", "-B", x, "-o", out(tag + mode), "--flagstat"] + extra + argv) == 0
            assert "Library size: %d mapped reads (%d primary)" % (w[6, 0], w[7, 0]) in capsys.readouterr().out
            assert read(out(tag + mode) + ".flagstat.txt") == want, (tag, mode)
            if mode in ("b", "nb"):        # (with the flag and without: the same .SpliSER.tsv, byte for byte)
                assert cli.main(["process", "-B", x, "-o", out(tag + mode + "_bare")] + extra + argv) == 0
                assert read(out(tag + mode) + ".SpliSER.tsv") == read(out(tag + mode + "_bare") + ".SpliSER.tsv"), (tag, mode)
                assert not os.path.exists(out(tag + mode + "_bare") + ".flagstat.txt")
    assert read(out("a.dev.txt")) != read(out("all.dev.txt"))
