"""The hand-built DEFLATE cases of deflatecases.py through the inflate and CRC32 kernels (spl_inflate.hip) on the card: every named
case and the FULL distance x length x phase sweep of the copying kernel in one image, with either decoding kernel, each refusal
between two legal blocks; the same image with less token room than the stride; and whole BAM files whose every BGZF block the hand
writer made from a perverse parse of the real record bytes.  test_deflate_cases_host.py has shown every case to end with a status
under the wave emulator, which bounds-checks every access of the same source, before any of them comes here."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

import deflatecases as dc
from spliser_amd import native, samio

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_IMAGE = {}


def _image():
    if not _IMAGE:
        cases = dc.refusals_between_legal(dc.named_cases() + dc.sweep(True))
        for k, c in enumerate(cases):
            if c.kind != "legal":
                assert cases[k - 1].kind == "legal" and cases[k + 1].kind == "legal"
        _IMAGE["cases"] = cases
        _IMAGE["image"] = dc.image_of(cases)
    return (_IMAGE["cases"],) + _IMAGE["image"]


def _device(cases, image, blocks, total):
    d_image = torch.from_numpy(np.frombuffer(image, np.uint8).copy()).to("cuda:0")      # (image_of has put SPL_Z_IMAGE_PAD zeros behind)
    d_blocks = torch.from_numpy(blocks.view(np.int64)).to("cuda:0")
    d_out = torch.full((total + 128,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_status = torch.full((len(cases),), -1, dtype=torch.int32, device="cuda:0")
    return d_image, d_blocks, d_out, d_status


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("dense", ["0", "1"])
def test_every_case_and_the_full_sweep_in_one_image(monkeypatch, dense):
    monkeypatch.setenv("SPL_Z_DENSE", dense)
    native.build()
    lib = native.lib()
    cases, image, blocks, starts, total = _image()
    n = len(cases)
    assert n > 14560
    d_image, d_blocks, d_out, d_status = _device(cases, image, blocks, total)
    lib.spl_dev_inflate_work_bytes.restype = ctypes.c_size_t
    d_work = torch.zeros(lib.spl_dev_inflate_work_bytes(ctypes.c_uint32(n)), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert lib.spl_dev_launch_inflate(_p(d_image), _p(d_blocks), ctypes.c_uint32(n), _p(d_out), _p(d_status), _p(d_work), ctypes.c_void_p(0)) == 0
    assert lib.spl_dev_launch_crc32(_p(d_out), _p(d_blocks), ctypes.c_uint32(n), _p(d_status), ctypes.c_void_p(0)) == 0
    torch.cuda.synchronize()
    status, got = d_status.cpu().numpy().view(np.uint32), d_out.cpu().numpy().tobytes()
    for k, c in enumerate(cases):
        dc.check(c, status[k], got[starts[k]:starts[k] + len(c.data)])
    assert got[total:] == b"\xa5" * 128                   # nothing written behind the last block


@pytest.mark.parametrize("stride", [1024, 8192])
@pytest.mark.parametrize("dense", [0, 1])
def test_less_token_room_than_the_stride(monkeypatch, dense, stride):
    """decode3 / copy2 with `stride` bytes of token room a block, told which decoding kernel to take: per block SPL_Z_TOKENS or what
    the case expects, nothing behind the output or behind the work space."""
    monkeypatch.delenv("SPL_Z_DENSE", raising=False)
    native.build()
    lib = native.lib()
    cases, image, blocks, starts, total = _image()
    n = len(cases)
    d_image, d_blocks, d_out, d_status = _device(cases, image, blocks, total)
    lib.spl_dev_inflate_work_bytes2.restype = ctypes.c_size_t
    n_work = lib.spl_dev_inflate_work_bytes2(ctypes.c_uint32(n), ctypes.c_uint32(stride))
    d_work = torch.full((n_work + 4096,), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert lib.spl_dev_launch_inflate_decode3(_p(d_image), _p(d_blocks), ctypes.c_uint32(n), _p(d_status), _p(d_work), ctypes.c_uint32(stride),
                                              ctypes.c_uint32(dense), ctypes.c_void_p(0)) == 0
    assert lib.spl_dev_launch_inflate_copy2(_p(d_blocks), ctypes.c_uint32(n), _p(d_out), _p(d_status), _p(d_work), ctypes.c_uint32(stride), ctypes.c_void_p(0)) == 0
    assert lib.spl_dev_launch_crc32(_p(d_out), _p(d_blocks), ctypes.c_uint32(n), _p(d_status), ctypes.c_void_p(0)) == 0
    torch.cuda.synchronize()
    status, got = d_status.cpu().numpy().view(np.uint32), d_out.cpu().numpy().tobytes()
    n_ok = 0
    for k, c in enumerate(cases):
        if status[k] == dc.TOKENS:
            assert 2 * len(c.data) > stride - 64, c.name  # (a byte of output is two bytes of tokens at most: not refused for nothing)
            continue
        dc.check(c, status[k], got[starts[k]:starts[k] + len(c.data)])
        n_ok += status[k] == dc.OK
    assert n_ok > 1000
    assert got[total:] == b"\xa5" * 128
    assert bytes(d_work[n_work:].cpu().numpy().tobytes()) == b"\xee" * 4096


@pytest.fixture(scope="module")
def ctx():
    native.build()
    with native.Context(0) as c:
        yield c


@pytest.mark.parametrize("window", [None, "3"])
@pytest.mark.parametrize("variant", dc.PERVERSE)
def test_bam_files_of_perverse_blocks(ctx, tmp_path, monkeypatch, variant, window):
    """Legal files: the device path must TAKE them (a fall-back to the host would hide a failure), and give what the host decoder
    gives and what was written.  Blocks stay below 64 KiB: payloads of 48 KiB, and a stored block where a parse still outgrows it --
    one block in ten at most."""
    from test_bam_decode import _random_sets
    from test_gpu_bam_device import _both
    made = {"blocks": 0, "stored": 0}

    def block(payload, level):
        data = dc.perverse_deflate(payload, variant) if payload else b"\x03\x00"
        made["blocks"] += 1
        if len(data) + 26 > 0x10000:
            made["stored"] += 1
            comp = zlib.compressobj(0, zlib.DEFLATED, -15)
            data = comp.compress(payload) + comp.flush()
        header = struct.pack("<BBBBIBBHBBHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 0x42, 0x43, 2, len(data) + 25)
        return header + data + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload) & 0xFFFFFFFF)
    monkeypatch.setattr(samio, "_bgzf_block", block)
    monkeypatch.setattr(samio, "_BGZF_BLOCK", 0xC000)
    if window:
        monkeypatch.setenv("SPL_INFLATE_WINDOW_BLOCKS", window)
    names, sets = _random_sets(31, 4_000, 2)
    path = str(tmp_path / "p.bam")
    samio.write_bam(path, names, [10 ** 8] * 2, [(c, sets[c]) for c in names], with_seq=True)
    assert made["blocks"] >= 5 and made["stored"] * 10 <= made["blocks"], made
    assert _both(path, ctx, names, sets) is True
