"""Canvas.bgzf_inflate (canvas_amd/csrc/inflate.hip) against zlib: every stream of tests/deflate_cases.py, one call each for the hand-built cases, zlib's own output
with the fixture BAM's blocks, and the 2000 mutations.  Status 0 exactly where zlib's raw inflate accepts the stream for its recorded size, zlib's bytes there, the
canary pattern everywhere outside the destination ranges of accepted blocks (a failed block leaves its range alone in this build, which the contract does not promise:
only the bytes OUTSIDE it are checked), and h_info as the statuses say.  One wave of 64 lanes per block."""
import functools

import numpy as np
import pytest

import deflate_cases as D
from gpu_common import get_canvas, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cv():
    return get_canvas()


@functools.lru_cache(maxsize=None)
def expected(kind):
    cases = {"hand": D.hand_cases, "zlib": D.zlib_cases, "mutations": D.mutations}[kind]()
    return cases, [D.expected_status(c[1], c[2]) for c in cases]


def canary(n):
    return ((np.arange(n, dtype=np.int64) * 7 + 3) & 0xFF).astype(np.uint8)


def run(cv, cases, want=None, pad_src=0, pad_dst=0, src_shift=0, dst_shift=0, tail=64, blocks=None, want_info=True, dst_size=None):
    """-> (dst as numpy, status as numpy).  `want`: expected_status per case (computed when None)"""
    want = [D.expected_status(c[1], c[2]) for c in cases] if want is None else want
    src, packed, dsize = D.pack(cases, pad_src, pad_dst)
    if blocks is None:
        blocks = packed
        blocks["src_offset"] += src_shift
        blocks["dst_offset"] += dst_shift
    src = np.frombuffer(b"\x5a" * src_shift + src, np.uint8).copy()
    dsize = dst_shift + dsize + tail if dst_size is None else dst_size
    before = canary(dsize)
    dst = to_dev(before, cv.device)
    out, status, info = cv.bgzf_inflate(to_dev(src, cv.device) if len(src) else to_dev(np.zeros(1, np.uint8), cv.device)[:0], blocks, out=dst, want_info=want_info)
    if not want_info:
        assert info is None
        cv.synchronize()
    got, st = out.cpu().numpy(), status.cpu().numpy()[:len(cases)]
    exp, checked, good_bytes, first = before.copy(), np.ones(dsize, bool), 0, -1
    for i, (b, (ok, data, refused)) in enumerate(zip(blocks, want)):
        assert (st[i] == 0) == ok and (st[i] == 1) == refused, (cases[i][0], int(st[i]))
        lo, n = int(b["dst_offset"]), int(b["out_bytes"])
        if ok:
            exp[lo:lo + n] = np.frombuffer(data, np.uint8)
            good_bytes += n
        else:
            first = i if first < 0 else first
            if not refused:
                checked[lo:lo + n] = False          # its own bytes are unspecified
    bad = np.nonzero((got != exp) & checked)[0]
    assert len(bad) == 0, ("first differing byte", int(bad[0]), len(bad))
    if want_info:
        assert info.tolist() == [len(cases), int((st != 0).sum()), good_bytes, first]
    return got, st


def test_hand_built_cases(cv):
    cases, want = expected("hand")
    got, st = run(cv, cases, want, pad_dst=3)
    for (name, s, o, accepted), code in zip(cases, st):
        assert (code == 0) == (accepted and len(s) <= D.LIMIT), name


def test_zlib_output_and_the_fixture_bam(cv):
    cases, want = expected("zlib")
    got, st = run(cv, cases, want, pad_src=1, pad_dst=1)
    assert (st == 0).sum() > 200 and (st == 1).sum() > 0


def test_mutations(cv):
    cases, want = expected("mutations")
    accepted = sum(ok for ok, data, refused in want)
    assert accepted >= 100 and len(cases) - accepted >= 100
    run(cv, cases, want, pad_dst=2)


def some_cases(n):
    """n cases, good and bad mixed, none large"""
    pool = [c for c in D.hand_cases() if len(c[1]) < 600 and c[2] < 600]
    return [pool[(5 * i) % len(pool)] for i in range(n)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_block_counts(cv, n):
    got, st = run(cv, some_cases(n))
    assert len(st) == n


@pytest.mark.parametrize("r", range(8))
def test_offsets_at_every_residue(cv, r):
    """block 0 starts at residue r (source) and (3 r + 1) mod 8 (destination) of the allocations; the blocks behind it at whatever their lengths give"""
    cases = some_cases(24) + [c for c in D.zlib_cases() if c[0] in ("zlib 4097 text level 6 default", "zlib 65536 text level 9 default")]
    run(cv, cases, src_shift=r, dst_shift=(3 * r + 1) % 8)
    run(cv, cases, src_shift=r, dst_shift=(3 * r + 1) % 8, pad_dst=r + 8)


def test_a_failed_block_between_two_good_ones(cv):
    by = {c[0]: c for c in D.hand_cases()}
    good1, good2 = by["overlap: distance 63 length 258"], by["fixed distance code 17: 385 and 512"]
    for bad in ("overrun by one byte from a match", "one byte short of out_bytes", "distance one more than the bytes produced", "fixed literal/length symbol 287",
                "input ends inside extra bits", "stored length beyond out_bytes"):
        got, st = run(cv, [good1, by[bad], good2], dst_shift=5)      # adjacent ranges: no byte between them
        assert st.tolist()[0] == 0 and st[1] != 0 and st[2] == 0


def test_descriptor_errors(cv):
    cases = some_cases(6)
    src, blocks, dsize = D.pack(cases)
    nsrc, want = len(src), [D.expected_status(c[1], c[2]) for c in cases]
    refused = (False, b"", True)

    def go(i, dst_size=dsize, **fields):
        b, w = blocks.copy(), list(want)
        for k, v in fields.items():
            b[i][k] = v
        w[i] = refused
        run(cv, cases, w, blocks=b, dst_size=dst_size, tail=0)

    last = len(cases) - 1
    go(last, src_bytes=int(blocks[last]["src_bytes"]) + 1)                     # one byte behind the source
    go(2, src_offset=nsrc + 1, src_bytes=0)
    go(2, src_offset=nsrc - 1, src_bytes=2)
    go(2, src_offset=(1 << 64) - 1, src_bytes=2)                               # no wrap-around
    go(3, dst_offset=dsize - int(blocks[3]["out_bytes"]) + 1)                  # one byte behind the destination
    go(3, dst_offset=dsize + 1, out_bytes=0)
    go(3, dst_offset=(1 << 64) - 1, out_bytes=2)
    go(1, src_offset=0, src_bytes=65537)
    go(1, out_bytes=65537, dst_offset=0, dst_size=70000)
    # exactly at the ends: accepted as a descriptor
    run(cv, cases, want, blocks=blocks.copy(), dst_size=dsize, tail=0)


def test_queued_form_and_repeat(cv):
    cases = some_cases(40) + [c for c in D.zlib_cases() if c[0] == "zlib 65536 text level 6 default"]
    a, sa = run(cv, cases)
    b, sb = run(cv, cases, want_info=False)
    c, sc = run(cv, cases)
    assert (sa == sb).all() and (sa == sc).all() and (a == b).all() and (a == c).all()


def test_descriptors_on_the_device_and_created_outputs(cv):
    import torch
    cases = some_cases(10)
    src, blocks, dsize = D.pack(cases)
    out, status, info = cv.bgzf_inflate(to_dev(np.frombuffer(src, np.uint8).copy(), cv.device), blocks)
    dev_blocks = torch.from_numpy(blocks.view(np.uint8).reshape(-1, 24).copy()).to(cv.device)
    out2, status2, info2 = cv.bgzf_inflate(to_dev(np.frombuffer(src, np.uint8).copy(), cv.device), dev_blocks, out=torch.zeros_like(out))
    assert info.tolist() == info2.tolist() and torch.equal(status, status2)
    for b, s, c in zip(blocks, status.cpu().numpy(), cases):
        if s == 0:
            lo, n = int(b["dst_offset"]), int(b["out_bytes"])
            assert out[lo:lo + n].cpu().numpy().tobytes() == out2[lo:lo + n].cpu().numpy().tobytes() == D.zlib_verdict(c[1], c[2])[1]


def test_call_level_errors(cv):
    """CANVAS_ERR_INVALID behind a valid context: negative nblocks, each buffer NULL with nblocks = 1; nblocks = 0 is OK with NULL buffers and launches nothing.
    A refused call names itself in canvas_last_error and touches neither the statuses nor the destination."""
    import ctypes as C
    import torch
    case = next(c for c in D.hand_cases() if c[0] == "two stored blocks")
    src, blocks, dsize = D.pack([case])
    d_src = to_dev(np.frombuffer(src, np.uint8).copy(), cv.device)
    d_blk = to_dev(blocks.view(np.uint8).reshape(-1).copy(), cv.device)
    d_dst = to_dev(canary(dsize + 16), cv.device)
    d_st = torch.full((4,), 77, dtype=torch.int32, device=cv.device)
    torch.cuda.synchronize()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def call(n, s=ptr(d_src), b=ptr(d_blk), d=ptr(d_dst), st=ptr(d_st), want_info=True):
        info = np.full(4, -5, np.int64)
        rc = cv.lib.canvas_bgzf_inflate(cv.ctx, s, C.c_uint64(len(src)), b, C.c_int64(n), d, C.c_uint64(dsize + 16), st, info.ctypes.data_as(C.c_void_p) if want_info else None)
        return rc, info.tolist()

    def untouched():
        cv.synchronize()
        return d_st.cpu().tolist() == [77] * 4 and (d_dst.cpu().numpy() == canary(dsize + 16)).all()

    for kw in (dict(n=-1), dict(n=-(1 << 40)), dict(n=1, s=None), dict(n=1, b=None), dict(n=1, d=None), dict(n=1, st=None), dict(n=1, s=None, want_info=False)):
        rc, info = call(**kw)
        assert rc == -1 and info == [-5] * 4, (kw, rc, info)
        assert b"canvas_bgzf_inflate" in cv.lib.canvas_last_error(cv.ctx), kw
        assert untouched(), kw
    for kw in (dict(n=0, s=None, b=None, d=None, st=None), dict(n=0)):
        rc, info = call(**kw)
        assert rc == 0 and info == [0, 0, 0, -1] and untouched(), (kw, rc, info)
    assert call(0, s=None, b=None, d=None, st=None, want_info=False)[0] == 0 and untouched()
    # ... and the same buffers in a call that is taken
    rc, info = call(1)
    cv.synchronize()
    assert rc == 0 and info == [1, 0, 11, -1] and d_st.cpu().tolist() == [0, 77, 77, 77] and d_dst[:11].cpu().numpy().tobytes() == b"hello world"
    assert (d_dst[11:].cpu().numpy() == canary(dsize + 16)[11:]).all()
