"""Canvas.bgzf_crc32 (canvas_amd/csrc/crc.hip) against zlib.crc32: the fixture BAM behind Canvas.bgzf_inflate, and synthetic blocks placed straight into the destination,
back to back (a kernel that reads one byte beyond a block's range picks up its neighbour's and fails), with the source built as stream || trailer by deflate_cases.pack.
Everything is an integer: crc[i] is zlib's value of the bytes present, status[i] says how it compares with the trailer word, and info is what the statuses say."""
import functools
import random
import struct
import zlib

import numpy as np
import pytest

import crc_cases as CC
import deflate_cases as D
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu
OK, MISMATCH, DESCRIPTOR, SKIPPED = 0, 1, 2, 3


@pytest.fixture(scope="module")
def cv():
    cv = get_canvas()
    from canvas_amd import lib as L
    assert (L.CRC_OK, L.CRC_MISMATCH, L.CRC_DESCRIPTOR, L.CRC_SKIPPED) == (OK, MISMATCH, DESCRIPTOR, SKIPPED)
    return cv


def trailer(data, flip=0):
    return struct.pack("<I", zlib.crc32(data) ^ flip)


def layout(datas, flips=None, shift=0):
    """-> (src bytes, descriptors, dst bytes): block i is datas[i] at the running offset from `shift` on, its source i % 4 bytes of stream and the trailer word behind them"""
    flips = flips or [0] * len(datas)
    src, blocks, dsize = D.pack([("block %d" % i, b"\x03\x00\x5a"[:i % 4] + trailer(d, f), len(d)) for i, (d, f) in enumerate(zip(datas, flips))])
    blocks["src_bytes"] -= 4
    blocks["dst_offset"] += shift
    return src, blocks, b"\x99" * shift + b"".join(datas)


def dev(cv, b):
    a = np.frombuffer(bytes(b), np.uint8).copy()
    return to_dev(a if len(a) else np.zeros(1, np.uint8), cv.device)[:len(a)]


def go(cv, src, blocks, dst, want_status=None, want_crc=None, **kw):
    """one call with the statuses and sums checked: want_crc[i] None = a block that is not summed"""
    import torch
    n = len(blocks)
    status = torch.full((n + 2,), 77, dtype=torch.int32, device=cv.device)
    crc = torch.full((n + 2,), 0x55, dtype=torch.int32, device=cv.device)
    queued = kw.get("want_info") is False
    c, s, info = cv.bgzf_crc32(dev(cv, src) if src is not None else None, blocks, dst if hasattr(dst, "numel") else dev(cv, dst), crc=crc, status=status, **kw)
    if queued:
        assert info is None
        cv.synchronize()
    got_c, got_s = c.cpu().numpy().view(np.uint32), s.cpu().numpy()
    assert got_s[n:].tolist() == [77, 77] and got_c[n:].tolist() == [0x55, 0x55]          # nothing behind the blocks is written
    got_c, got_s = got_c[:n].tolist(), got_s[:n].tolist()
    if want_status is not None:
        assert got_s == list(want_status), [(i, a, b) for i, (a, b) in enumerate(zip(got_s, want_status)) if a != b][:5]
    if want_crc is not None:
        want = [0 if w is None else w for w in want_crc]
        assert got_c == want, [(i, int(blocks[i]["out_bytes"]), hex(a), hex(b)) for i, (a, b) in enumerate(zip(got_c, want)) if a != b][:5]
    if not queued:
        bad = [i for i, st in enumerate(got_s) if st not in (OK, SKIPPED)]
        summed = sum(int(blocks[i]["out_bytes"]) for i, st in enumerate(got_s) if st in (OK, MISMATCH))
        assert info.tolist() == [n, len(bad), summed, bad[0] if bad else -1]
    return got_c, got_s, info


@functools.lru_cache(maxsize=None)
def every_length():
    """the blocks of crc_cases with zlib's sums, made once"""
    datas = [c[2] for c in CC.blocks_of_every_length()]
    return datas, [zlib.crc32(d) for d in datas]


def test_fixture_bam(cv):
    import canvas_amd
    raw = open(D.FIXTURE_BAM, "rb").read()
    blocks, scan = canvas_amd.bgzf_scan(raw)
    src = dev(cv, raw)
    out, status, info = cv.bgzf_inflate(src, blocks)
    assert info[1] == 0
    want = [zlib.crc32(D.zlib_verdict(s, o)[1]) for s, o in D.bam_blocks()]
    crc, st, info = cv.bgzf_crc32(src, blocks, out, inflate_status=status)
    n, total = len(blocks), int(blocks["out_bytes"].sum())
    assert n == len(want) > 1 and info.tolist() == [n, 0, total, -1]
    assert st.cpu().numpy()[:n].tolist() == [OK] * n and crc.cpu().numpy().view(np.uint32)[:n].tolist() == want
    # ... and the descriptors as a device tensor
    import torch
    crc2, st2, info2 = cv.bgzf_crc32(src, torch.from_numpy(blocks.view(np.uint8).reshape(-1, 24).copy()).to(cv.device), out)
    assert info2.tolist() == info.tolist() and torch.equal(crc2.view(torch.int32), crc.view(torch.int32)) and torch.equal(st2, st)


@pytest.mark.parametrize("shift", range(16))
def test_lengths_at_every_offset(cv, shift):
    """block 0 starts `shift` bytes past a 16-byte boundary, the blocks behind it wherever their lengths put them: every head and tail of the 16-byte loads"""
    datas, want = every_length()
    src, blocks, dst = layout(datas, shift=shift)
    d = dev(cv, dst)
    assert d.data_ptr() % 16 == 0 and len(set(int(o) % 16 for o in blocks["dst_offset"])) == 16
    go(cv, src, blocks, d, [OK] * len(datas), want)


def test_mismatches(cv):
    rng = random.Random(3)
    datas = [rng.randbytes(n) for n in (700, 5000, 33, 65536, 1)]
    src, blocks, dst = layout(datas, flips=[0, 1 << 19, 0, 0, 0])          # block 1: the trailer word off by one bit
    dst = bytearray(dst)
    dst[int(blocks[3]["dst_offset"]) + 40000] ^= 0x10                        # block 3: one data byte flipped after the trailer was computed
    present = [zlib.crc32(bytes(dst[int(b["dst_offset"]):int(b["dst_offset"]) + int(b["out_bytes"])])) for b in blocks]
    assert present[3] != zlib.crc32(datas[3]) and present[1] == zlib.crc32(datas[1])
    c, s, info = go(cv, src, blocks, dst, [OK, MISMATCH, OK, MISMATCH, OK], present)
    assert info[1] == 2 and info[3] == 1
    # compute only: nothing is compared
    go(cv, None, blocks, dst, [OK] * 5, present)


def test_descriptors(cv):
    rng = random.Random(4)
    datas = [rng.randbytes(n) for n in (300, 65536, 17, 1000)]
    want = [zlib.crc32(d) for d in datas]
    src, blocks, dst = layout(datas)

    def one(i, b=None, src=src, dst=dst):
        st, w = [OK] * 4, list(want)
        st[i], w[i] = DESCRIPTOR, None
        c, s, info = go(cv, src, blocks if b is None else b, dst, st, w)
        assert info[1] == 1 and info[3] == i

    b = blocks.copy()
    b[1]["out_bytes"] = 65537
    one(1, b, dst=dst + b"\x00" * 8)
    one(3, dst=dst[:-1])                                                     # the data range ends one byte past dst_nbytes
    one(3, src=src[:-1])                                                     # the trailer ends one byte past src_nbytes
    b = blocks.copy()
    b[2]["dst_offset"] = (1 << 64) - 1                                       # no wrap-around
    one(2, b)
    b = blocks.copy()
    b[0]["src_offset"] = (1 << 64) - 2
    one(0, b)
    go(cv, src[:-1], blocks, dst[:-1], [OK, OK, OK, DESCRIPTOR], want[:3] + [None])
    go(cv, None, blocks, dst, [OK] * 4, want)                                # without a source the trailers are not looked for
    go(cv, src, blocks, dst, [OK] * 4, want)                                 # exactly at the ends: accepted


def test_skipping_a_block_the_inflater_refused(cv):
    by = {c[0]: c for c in D.hand_cases()}
    cases = [by["overlap: distance 63 length 258"], by["one byte short of out_bytes"], by["fixed distance code 17: 385 and 512"]]
    data = [D.zlib_verdict(c[1], c[2])[1] for c in cases]
    assert data[0] and data[2] and not D.zlib_verdict(cases[1][1], cases[1][2])[0]
    src, blocks, dsize = D.pack([(c[0], c[1] + trailer(d or b""), c[2]) for c, d in zip(cases, data)])
    blocks["src_bytes"] -= 4
    s = dev(cv, src)
    out, status, info = cv.bgzf_inflate(s, blocks)
    assert info[1] == 1 and info[3] == 1
    c, st, info = go(cv, src, blocks, out, [OK, SKIPPED, OK], [zlib.crc32(data[0]), None, zlib.crc32(data[2])], inflate_status=status)
    assert info.tolist() == [3, 0, len(data[0]) + len(data[2]), -1]
    # without the statuses the block is summed like any other
    c, st, info = go(cv, src, blocks, out)
    assert st[0] == OK and st[2] == OK and st[1] in (OK, MISMATCH)


def test_small_calls(cv):
    empty = np.zeros(0, D.pack([])[1].dtype)
    c, s, info = go(cv, b"", empty, b"\x00")
    assert info.tolist() == [0, 0, 0, -1]
    go(cv, None, empty, b"\x00", want_info=False)
    src, blocks, dst = layout([b""])
    c, s, info = go(cv, src, blocks, b"\x00", [OK], [0])
    assert info.tolist() == [1, 0, 0, -1]
    src, blocks, dst = layout([b""], flips=[1])                              # an empty block sums to 0 whatever its trailer says
    go(cv, src, blocks, b"\x00", [MISMATCH], [0])


def test_many_small_blocks(cv):
    rng = random.Random(5)
    datas = [rng.randbytes(1 + i % 40) for i in range(3000)]
    flips = [1 if i in (0, 1499, 2999) else 0 for i in range(3000)]
    src, blocks, dst = layout(datas, flips=flips, shift=5)
    c, s, info = go(cv, src, blocks, dst, [MISMATCH if f else OK for f in flips], [zlib.crc32(d) for d in datas])
    assert info[1] == 3 and info[3] == 0


def test_queued_form(cv):
    datas, want = every_length()
    src, blocks, dst = layout(datas, shift=3)
    a = go(cv, src, blocks, dst, [OK] * len(datas), want)
    b = go(cv, src, blocks, dst, [OK] * len(datas), want, want_info=False)
    c = go(cv, src, blocks, dst, [OK] * len(datas), want)
    assert a[:2] == b[:2] == c[:2]
