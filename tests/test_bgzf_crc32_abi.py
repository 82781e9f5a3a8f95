"""canvas_bgzf_crc32 at the C ABI, without a GPU: the status codes of the header against those of canvas_amd.lib, the symbol, and the calls that are refused before any
device work.  (The arithmetic runs on the host in tests/test_crc32_host.py, the kernel in tests/test_bgzf_crc32_gpu.py.)"""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import build
    so, _ = build.build()
    lib = ctypes.CDLL(so)
    lib.canvas_bgzf_crc32.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.canvas_bgzf_crc32.restype = ctypes.c_int32
    return lib


def test_codes_of_the_header():
    from canvas_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    codes = dict((n, int(v)) for n, v in re.findall(r"#define (CANVAS_CRC_\w+) (\d+)", hdr))
    assert codes == dict(CANVAS_CRC_OK=L.CRC_OK, CANVAS_CRC_MISMATCH=L.CRC_MISMATCH, CANVAS_CRC_DESCRIPTOR=L.CRC_DESCRIPTOR, CANVAS_CRC_SKIPPED=L.CRC_SKIPPED)
    assert [L.CRC_OK, L.CRC_MISMATCH, L.CRC_DESCRIPTOR, L.CRC_SKIPPED] == [0, 1, 2, 3]


def test_declared_listed_and_bound():
    from canvas_amd import Canvas
    from canvas_amd.lib import ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    assert "canvas_bgzf_crc32" in ABI_SYMBOLS and callable(Canvas.bgzf_crc32)
    assert hdr.index("int32_t canvas_bgzf_scan(") < hdr.index("int32_t canvas_bgzf_crc32(") < hdr.index("int32_t canvas_bam_frame(")
    assert "canvas_bgzf_crc32(IntPtr ctx" in open(os.path.join(ROOT, "hosts", "CanvasHip.cs")).read()


def test_crc32_refuses_without_a_context(lib):
    buf = (ctypes.c_uint8 * 64)()
    info = (ctypes.c_int64 * 4)(-5, -5, -5, -5)
    for n in (-1, 0, 1):
        assert lib.canvas_bgzf_crc32(None, buf, 64, buf, n, buf, 64, buf, buf, buf, info) == -1      # CANVAS_ERR_INVALID
        assert lib.canvas_bgzf_crc32(None, None, 0, buf, n, buf, 64, None, buf, buf, None) == -1
    assert list(info) == [-5] * 4
