"""canvas_bgzf_inflate / canvas_bgzf_scan at the C ABI, without a GPU: the descriptor's layout, the status and stop codes of the header, the calls that are refused
before any device work, and the block walk through ctypes and through canvas_amd.bgzf_scan."""
import ctypes
import os
import re
import struct
import zlib

import numpy as np
import pytest

import deflate_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import build
    so, _ = build.build()
    lib = ctypes.CDLL(so)
    lib.canvas_bgzf_scan.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.canvas_bgzf_inflate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def test_descriptor_is_24_bytes():
    from canvas_amd.lib import BGZF_BLOCK
    assert BGZF_BLOCK.itemsize == 24 and D.pack([])[1].dtype == BGZF_BLOCK
    assert [BGZF_BLOCK.fields[n][1] for n in ("src_offset", "dst_offset", "src_bytes", "out_bytes")] == [0, 8, 16, 20]
    hdr = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    assert re.search(r"typedef struct \{ uint64_t src_offset; uint64_t dst_offset; uint32_t src_bytes; uint32_t out_bytes; \} canvas_bgzf_block;", hdr)


def test_codes_of_the_header():
    from canvas_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    codes = dict((n, int(v)) for n, v in re.findall(r"#define (CANVAS_(?:INFLATE|BGZF_SCAN)_\w+) (\d+)", hdr))
    assert codes == dict(CANVAS_INFLATE_OK=0, CANVAS_INFLATE_DESCRIPTOR=1, CANVAS_INFLATE_HEADER=2, CANVAS_INFLATE_INPUT=3, CANVAS_INFLATE_OVERRUN=4,
                         CANVAS_INFLATE_SHORT=5, CANVAS_INFLATE_DISTANCE=6, CANVAS_INFLATE_CODE=7, CANVAS_BGZF_SCAN_LIMIT=0, CANVAS_BGZF_SCAN_END=1, CANVAS_BGZF_SCAN_DAMAGED=2)
    assert [L.INFLATE_OK, L.INFLATE_DESCRIPTOR, L.INFLATE_HEADER, L.INFLATE_INPUT, L.INFLATE_OVERRUN, L.INFLATE_SHORT, L.INFLATE_DISTANCE, L.INFLATE_CODE] == list(range(8))
    assert [L.BGZF_SCAN_LIMIT, L.BGZF_SCAN_END, L.BGZF_SCAN_DAMAGED] == [0, 1, 2]


def test_inflate_refuses_without_a_context(lib):
    buf = (ctypes.c_uint8 * 64)()
    info = (ctypes.c_int64 * 4)()
    for n in (-1, 0, 1):
        assert lib.canvas_bgzf_inflate(None, buf, 64, buf, n, buf, 64, buf, info) == -1      # CANVAS_ERR_INVALID


def test_scan_refusals(lib):
    raw = open(D.FIXTURE_BAM, "rb").read()
    blocks = np.zeros(4, D.pack([])[1].dtype)
    info = np.zeros(4, np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.canvas_bgzf_scan(raw, len(raw), 0, 1 << 40, p(blocks), 4, None) == -1
    assert lib.canvas_bgzf_scan(None, len(raw), 0, 1 << 40, p(blocks), 4, p(info)) == -1
    assert lib.canvas_bgzf_scan(raw, len(raw), 0, 1 << 40, p(blocks), -1, p(info)) == -1
    assert lib.canvas_bgzf_scan(raw, len(raw), 0, 1 << 40, None, 4, p(info)) == -1
    assert lib.canvas_bgzf_scan(raw, len(raw), len(raw) + 1, 1 << 40, p(blocks), 4, p(info)) == -1
    assert lib.canvas_bgzf_scan(raw, len(raw), len(raw), 1 << 40, p(blocks), 4, p(info)) == 0 and info.tolist() == [0, len(raw), 0, 1]
    assert lib.canvas_bgzf_scan(None, 0, 0, 1 << 40, None, 0, p(info)) == 0 and info.tolist() == [0, 0, 0, 0]


def test_scan_of_the_fixture_bam(lib):
    import canvas_amd
    raw = open(D.FIXTURE_BAM, "rb").read()
    want = D.bam_blocks()
    blocks, info = canvas_amd.bgzf_scan(raw)
    assert info.tolist() == [len(want), len(raw), sum(o for s, o in want), 1] and len(blocks) == len(want)
    at = 0
    for b, (stream, isize) in zip(blocks, want):
        assert raw[int(b["src_offset"]):int(b["src_offset"]) + int(b["src_bytes"])] == stream and int(b["out_bytes"]) == isize and int(b["dst_offset"]) == at
        assert D.zlib_verdict(stream, isize)[0]
        at += isize
    # in pieces: the next call starts where the last one stopped
    got, pos = [], 0
    while True:
        part, info = canvas_amd.bgzf_scan(np.frombuffer(raw, np.uint8), at=pos, max_out_bytes=100000)
        got += part.tolist()
        pos = int(info[1])
        if info[3] != 0:
            break
    assert info[3] == 1 and [(g[0], g[2], g[3]) for g in got] == [(int(b["src_offset"]), int(b["src_bytes"]), int(b["out_bytes"])) for b in blocks]
    # a file cut inside its last block
    part, info = canvas_amd.bgzf_scan(raw[:-9])
    assert info[3] == 2 and info[0] == len(want) - 1 and raw[int(info[1]):int(info[1]) + 4] == b"\x1f\x8b\x08\x04"
    # ctypes with a capacity below the file's blocks
    few = np.zeros(2, blocks.dtype)
    out = np.zeros(4, np.int64)
    assert lib.canvas_bgzf_scan(raw, len(raw), 0, 1 << 62, few.ctypes.data_as(ctypes.c_void_p), 2, out.ctypes.data_as(ctypes.c_void_p)) == 0
    assert out[0] == 2 and out[3] == 0 and (few == blocks[:2]).all()
    assert struct.calcsize("<QQII") == 24 and zlib.crc32(b"") == 0
