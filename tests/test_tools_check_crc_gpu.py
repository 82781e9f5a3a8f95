"""CANVAS_TOOL_CHECK_CRC=1: CanvasSNV, CanvasBin -c and CanvasBin -m Fragment hold the CRC32 of every BGZF block they inflate against the block's trailer, on the host
path (zlib's crc32 on the worker threads), with CANVAS_TOOL_DEVICE_INFLATE=1 and with CANVAS_TOOL_DEVICE_FRAME=1 (canvas_bgzf_crc32 behind canvas_bgzf_inflate).
The BAMs are those of tests/test_tools_device_inflate_gpu.py: blocks alternately at levels 0 and 6, an empty block in the middle, chunks of 64 KiB.  Two damaged copies
inflate well to the right sizes: (a) the CRC word of one block in the second half of chr1 off by one bit; (b) one data byte of a stored block flipped, stream and ISIZE
intact.  Off by default: without the variable file (a) reads as the intact file does.  With it the intact file gives the same files, stdout, messages and exit code, and
(a) and (b) end as the file with one corrupted deflate byte ends, the same way on the three paths."""
import os
import struct
import zlib

import pytest

import deflate_cases as D
import test_tools_device_inflate_gpu as TI
from test_tools_device_inflate_gpu import fragment_sample, hits_sample, snv_sample      # noqa: F401  (the module's fixtures, made again for this module)

pytestmark = pytest.mark.gpu
PATHS = [None, "CANVAS_TOOL_DEVICE_INFLATE", "CANVAS_TOOL_DEVICE_FRAME"]


@pytest.fixture(scope="module", autouse=True)
def built():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from canvas_amd import build
    build.build()


def crc_damaged(bam, kind, tmp_path):
    """one block in the second half of chr1's records whose stream still inflates to its ISIZE: "crc_word" = bit 11 of its CRC32 flipped; "data_byte" = a stored block
    with one of the bytes it holds changed"""
    raw = bytearray(open(bam, "rb").read())
    blocks, at = [], 0
    while at < len(raw):
        xlen, = struct.unpack_from("<H", raw, at + 10)
        size = struct.unpack_from("<H", raw, at + 12 + xlen - 2)[0] + 1          # (reblock_bam puts BC last)
        blocks.append((at, 12 + xlen, size))
        at += size
    for at, head, size in blocks[len(blocks) // 4:]:
        crc, isize = struct.unpack_from("<II", raw, at + size - 8)
        stored = size - head - 8 > isize                                         # (a stored block is longer than what it holds)
        if isize < 2000 or (kind == "data_byte" and not stored):
            continue
        assert zlib.crc32(D.zlib_verdict(bytes(raw[at + head:at + size - 8]), isize)[1]) == crc
        if kind == "crc_word":
            struct.pack_into("<I", raw, at + size - 8, crc ^ (1 << 11))
        else:
            raw[at + head + 5 + 1000] ^= 0x04                                    # behind the 5 bytes of the stored block's header
        ok, data = D.zlib_verdict(bytes(raw[at + head:at + size - 8]), isize)
        assert ok and zlib.crc32(data) != struct.unpack_from("<I", raw, at + size - 8)[0]
        break
    else:
        raise AssertionError("no block to damage")
    bad = str(tmp_path / ("%s_%s" % (kind, os.path.basename(bam))))
    open(bad, "wb").write(raw)
    open(bad + ".bai", "wb").write(open(bam + ".bai", "rb").read())
    return bad


def run(cmd, bam, path, check):
    """TI.run with the path and the check chosen through the environment it copies"""
    exe, args, outputs, chunk_var = cmd(bam)
    saved = dict(os.environ)
    for v in PATHS[1:] + ["CANVAS_TOOL_CHECK_CRC"]:
        os.environ.pop(v, None)
    if path == "CANVAS_TOOL_DEVICE_FRAME":
        os.environ[path] = "1"
    if check:
        os.environ["CANVAS_TOOL_CHECK_CRC"] = "1"
    try:
        return TI.run(exe, args, outputs, path == "CANVAS_TOOL_DEVICE_INFLATE", chunk_var)
    finally:
        os.environ.clear()
        os.environ.update(saved)


def command(tool, hits_sample, fragment_sample, snv_sample, tmp_path):
    """-> (bam, bam -> (executable, arguments, output files, the variable of the chunk size))"""
    if tool == "snv":
        d, bam, vcf = snv_sample
        out = str(tmp_path / "chr1.txt.gz")
        return bam, lambda b: (TI.SNV, ["-c", "chr1", "-v", vcf, "-b", b, "-o", out], [out, out + ".baf"], "CANVAS_SNV_CHUNK_BYTES")
    if tool == "bin_c":
        d, fa, bam = hits_sample
        out = str(tmp_path / "chr1.dat")
        return bam, lambda b: (TI.BIN, ["-b", b, "-r", fa, "-c", "chr1", "-o", out, "-d", "100", "-m", "3"], [out], "CANVAS_BIN_CHUNK_BYTES")
    d, fa, bed, bam = fragment_sample
    out = str(tmp_path / "out.binned")
    return bam, lambda b: (TI.BIN, ["-b", b, "-r", fa, "-n", bed, "-o", out, "-m", "Fragment", "-p"], [out], "CANVAS_BIN_CHUNK_BYTES")


def flagged(timing, path, check):
    want = ['"device_inflate": %d,' % (path is not None), '"device_frame": %d,' % (path == "CANVAS_TOOL_DEVICE_FRAME"), '"check_crc": %d, "crc_kernel_ms": ' % check]
    return bool(timing) and all(w in ln and ln.endswith("}") for ln in timing for w in want)


@pytest.mark.parametrize("tool", ["snv", "bin_c", "fragment"])
def test_intact_file_reads_the_same(tool, hits_sample, fragment_sample, snv_sample, tmp_path):
    bam, cmd = command(tool, hits_sample, fragment_sample, snv_sample, tmp_path)
    for path in PATHS:
        off, on = run(cmd, bam, path, False), run(cmd, bam, path, True)
        assert off[0] == 0 and all(off[3]) and on[:4] == off[:4], (path, on[:3], off[:3])
        assert flagged(off[4], path, 0) and flagged(on[4], path, 1), (path, off[4], on[4])
        if tool != "snv":
            assert all('"host_path": 0' in ln for ln in on[4]), on[4]


@pytest.mark.parametrize("kind", ["crc_word", "data_byte"])
@pytest.mark.parametrize("tool", ["snv", "bin_c", "fragment"])
def test_damaged_file_is_refused_on_request(tool, kind, hits_sample, fragment_sample, snv_sample, tmp_path):
    bam, cmd = command(tool, hits_sample, fragment_sample, snv_sample, tmp_path)
    bad = crc_damaged(bam, kind, tmp_path)
    refused = run(cmd, TI.damaged(bam, "deflate_byte", tmp_path), None, False)      # what the tool does with a block that does not inflate
    assert refused[0] != 0
    if kind == "crc_word":                                                          # off by default: nothing looks at the word
        intact = run(cmd, bam, None, False)
        for path in PATHS:
            off = run(cmd, bad, path, False)
            said = (off[0], off[1].replace(bad, bam), [m.replace(bad, bam) for m in off[2]], off[3])      # (the tools name their input)
            assert intact[0] == 0 and said == intact[:4] and flagged(off[4], path, 0), (path, off[:3])
    on = [run(cmd, bad, path, True) for path in PATHS]
    for path, r in zip(PATHS, on):
        assert r[0] == refused[0], (path, r[:3], refused[:3])
        assert all(f is None or g is not None for f, g in zip(r[3], refused[3])), path      # no output file beyond what that case leaves
        assert r[:4] == on[0][:4], (path, r[:3], on[0][:3])                           # the three paths agree
    if tool == "snv":
        assert any("a BGZF block fails its CRC32" in m for m in on[0][2]) and not any("does not inflate" in m for m in on[0][2])
