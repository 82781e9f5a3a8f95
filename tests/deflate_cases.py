"""Deflate streams for the tests of canvas_bgzf_inflate, shared by the CPU tests (test_deflate_cases.py holds this file to zlib, test_inflate_host.py runs the decoder
of canvas_amd/csrc/inflate_block.hpp on them under AddressSanitizer) and the GPU test (test_bgzf_inflate_gpu.py).

  W                a bit writer that assembles streams by hand: deflate packs fields LSB first and Huffman codes MSB first
  zlib_verdict     inflate_raw of canvas_amd/tools/bam_io.hpp restated: (accepted, bytes) of a stream that has to give exactly out_bytes
  hand_cases()     [(name, stream, out_bytes, accepted)]: each the smallest stream at which one rule of the contract can go wrong, with the verdict STATED
  zlib_cases()     [(name, stream, out_bytes)]: what zlib itself writes (sizes x data x levels x strategies) and every block of the fixture BAM; all valid
  mutations()      [(name, stream, out_bytes)]: 2000 streams, one to three bits of a valid one flipped; zlib alone decides (MUTATION_SEED: at least 100 either way)
A stream longer than 65536 bytes (zlib's level 0 or random data at 65536 bytes) cannot be a BGZF block: its descriptor is refused (expected_status)."""
import functools
import os
import random
import struct
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE_BAM = os.path.join(HERE, "golden", "ref_data", "single-end.bam")
MUTATION_SEED = 20261020
LIMIT = 65536


class W:
    def __init__(self):
        self.v, self.n = 0, 0

    def bits(self, value, n):                  # a field of n bits, least significant first
        assert 0 <= value < (1 << n) or n == 0
        self.v |= value << self.n
        self.n += n
        return self

    def huff(self, code, n):                   # a Huffman code of n bits, most significant first
        return self.bits(int(format(code, "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self):
        self.n = (self.n + 7) // 8 * 8
        return self

    def raw(self, data):
        assert self.n % 8 == 0
        self.v |= int.from_bytes(data, "little") << self.n
        self.n += 8 * len(data)
        return self

    def done(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def zlib_verdict(stream, out_bytes):
    """inflate_raw: Z_STREAM_END reached with exactly out_bytes written (one byte of room more than that tells an overrun from the end)"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(stream), out_bytes + 1)
    except zlib.error:
        return False, b""
    ok = d.eof and len(out) == out_bytes
    return ok, out if ok else b""


def expected_status(stream, out_bytes):
    """-> (accepted, bytes, descriptor refused)"""
    if len(stream) > LIMIT or out_bytes > LIMIT:
        return False, b"", True
    ok, out = zlib_verdict(stream, out_bytes)
    return ok, out, False


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [max(0, d // 2 - 1) for d in range(30)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def canon(lens):
    """symbol -> (code, length) of the canonical code (RFC 1951 3.2.2), also for sets that are no prefix code"""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for n in range(1, 17):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n] & ((1 << n) - 1), n)
            nxt[n] += 1
    return out


FIXED_LIT = canon([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canon([5] * 32)


def emit(w, lc, dc, ops):
    """int: a literal or any literal/length symbol; ("m", length, dist[, length symbol]): a match; ("d", symbol): a bare distance symbol; ("b", value, n): raw bits;
    "E": end of block"""
    for op in ops:
        if op == "E":
            w.huff(*lc[256])
        elif isinstance(op, int):
            w.huff(*lc[op])
        elif op[0] == "b":
            w.bits(op[1], op[2])
        elif op[0] == "d":
            w.huff(*dc[op[1]])
        else:
            length, dist = op[1], op[2]
            ls = op[3] if len(op) > 3 else (285 if length == 258 else 257 + max(i for i in range(29) if LBASE[i] <= length))
            w.huff(*lc[ls]).bits(length - LBASE[ls - 257], LEXT[ls - 257])
            d = max(j for j in range(30) if DBASE[j] <= dist)
            w.huff(*dc[d]).bits(dist - DBASE[d], DEXT[d])
    return w


def fixed(ops, final=1, w=None):
    w = w or W()
    w.bits(final, 1).bits(1, 2)
    return emit(w, FIXED_LIT, FIXED_DIST, ops)


def stored(data, final=1, w=None, nlen=None, length=None):
    w = w or W()
    n = len(data) if length is None else length
    w.bits(final, 1).bits(0, 2).align().bits(n, 16).bits((n ^ 0xFFFF) if nlen is None else nlen, 16)
    return w.raw(data)


def rle(lens):
    """the code-length symbols of a length list, greedy: [(symbol, extra value, first index, indices covered)]"""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            k = min(run, 138)
            out.append((18, k - 11, i, k) if k >= 11 else (17, k - 3, i, k))
            i += k
        elif v != 0 and run >= 4:
            k = min(run - 1, 6)
            out += [(v, 0, i, 1), (16, k - 3, i + 1, k)]
            i += 1 + k
        else:
            out.append((v, 0, i, 1))
            i += 1
    return out


CL_DEFAULT = [4] * 13 + [5] * 6                  # a complete code over all 19 code-length symbols


def dynamic(lit_lens, dist_lens, ops, final=1, w=None, hclen=19, cl_lens=None, seq=None, hlit=None, hdist=None):
    w = w or W()
    cl_lens = CL_DEFAULT if cl_lens is None else cl_lens
    w.bits(final, 1).bits(2, 2).bits(len(lit_lens) - 257 if hlit is None else hlit, 5).bits(len(dist_lens) - 1 if hdist is None else hdist, 5).bits(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.bits(cl_lens[s], 3)
    cc = canon(cl_lens)
    for item in (rle(list(lit_lens) + list(dist_lens)) if seq is None else seq):
        w.huff(*cc[item[0]])
        if item[0] >= 16:
            w.bits(item[1], {16: 2, 17: 3, 18: 7}[item[0]])
    return emit(w, canon(lit_lens), canon(dist_lens), ops)


def lens_of(n, **at):
    """n code lengths, zero but for s<symbol>=length"""
    out = [0] * n
    for k, v in at.items():
        out[int(k[1:])] = v
    return out


A, B = 97, 98
LIT3 = lens_of(258, s97=1, s256=2, s257=2)       # 'a', end of block, length 3: complete
RNG_BYTES = random.Random(7).randbytes(32768)


@functools.lru_cache(maxsize=None)
def hand_cases():
    c = []

    def add(name, w, out_bytes, accepted):
        c.append((name, w if isinstance(w, bytes) else w.done(), out_bytes, accepted))

    # ---- empty and stored
    add("BGZF EOF block", b"\x03\x00", 0, True)
    for n in (0, 1, 65535):
        add("stored %d" % n, stored((RNG_BYTES * 2)[:n]), n, True)
    add("the largest stored block a BGZF block holds", stored((RNG_BYTES * 2)[:65531]), 65531, True)
    w = stored((RNG_BYTES * 2)[:65536 - 259], w=fixed([A, ("m", 258, 1), "E"], final=0))
    add("a final stored block filling out_bytes 65536 behind a Huffman block", w, 65536, True)
    add("that stored block one byte past out_bytes 65536", stored((RNG_BYTES * 2)[:65536 - 258], w=fixed([A, ("m", 258, 1), "E"], final=0)), 65536, False)
    add("two stored blocks", stored(b"world", w=stored(b"hello ", final=0)), 11, True)
    for a in range(8):
        w = fixed([200] * a + ["E"], final=0)
        add("stored behind a Huffman block ending at bit %d" % (w.n % 8), stored(b"xyz", w=w), a + 3, True)
    assert sorted(x[0][-1] for x in c[-8:]) == list("01234567")
    add("stored LEN != ~NLEN", stored(b"abc", nlen=0xFFFD), 3, False)
    add("stored length beyond the input", stored(b"abcde", length=10), 10, False)
    add("stored length beyond out_bytes", stored(b"0123456789"), 9, False)
    add("BTYPE 3", W().bits(1, 1).bits(3, 2).bits(0, 13), 0, False)
    # ---- fixed codes
    add("fixed literals 0 143 144 255", fixed([0, 143, 144, 255, "E"]), 4, True)
    for i in range(29):
        lo, hi = LBASE[i], LBASE[i] + (1 << LEXT[i]) - 1
        add("fixed length code %d: %d and %d" % (257 + i, lo, hi), fixed([A, ("m", lo, 1, 257 + i), ("m", hi, 1, 257 + i), "E"]), 1 + lo + hi, True)
    for d in range(30):
        lo, hi = DBASE[d], DBASE[d] + (1 << DEXT[d]) - 1
        w = stored(RNG_BYTES[:hi], final=0)
        add("fixed distance code %d: %d and %d" % (d, lo, hi), fixed([("m", 3, lo), ("m", 3, hi), "E"], w=w), hi + 6, True)
    for s in (286, 287):
        add("fixed literal/length symbol %d" % s, fixed([A, s, ("b", 0, 5), "E"]), 4, False)
    for s in (30, 31):
        add("fixed distance symbol %d" % s, fixed([A, 257, ("d", s), "E"]), 4, False)
    # ---- matches
    add("distance 1 length 258", fixed([A, ("m", 258, 1), "E"]), 259, True)
    for d in range(1, 71):
        add("overlap: distance %d length 258" % d, fixed(list(range(33, 33 + d)) + [("m", 258, d), "E"]), d + 258, True)
    add("distance equal to the bytes produced", fixed([A, B, 99, ("m", 3, 3), "E"]), 6, True)
    add("distance one more than the bytes produced", fixed([A, B, 99, ("m", 3, 4), "E"]), 6, False)
    add("distance with nothing produced", fixed([("m", 3, 1), "E"]), 3, False)
    add("match across a deflate-block boundary", fixed([("m", 3, 3), "E"], w=fixed([A, B, 99, "E"], final=0)), 6, True)
    add("match across a stored block", fixed([("m", 5, 5), "E"], w=stored(b"hello", final=0)), 10, True)
    add("overrun by one byte from a match", fixed([A, ("m", 10, 1), "E"]), 10, False)
    add("overrun by one byte from a literal", fixed([A, B, 99, "E"]), 2, False)
    add("one byte short of out_bytes", fixed([A, B, 99, "E"]), 4, False)
    add("an empty stored block behind full output", stored(b"", w=fixed([A, "E"], final=0)), 1, True)
    # ---- dynamic codes
    add("dynamic HCLEN 19", dynamic(LIT3, [1, 1], [A, A, ("m", 3, 1), ("m", 3, 2), "E"]), 8, True)
    add("dynamic without repeat codes", dynamic(LIT3, [1, 1], [A, ("m", 3, 1), "E"], seq=[(v, 0) for v in LIT3 + [1, 1]]), 4, True)
    zeros258 = [(18, 127), (18, 109)]
    add("dynamic HCLEN 4", dynamic([0] * 257, [0], [("b", 0, 8)], hclen=4, cl_lens=lens_of(19, s16=2, s17=2, s18=2, s0=2), seq=zeros258), 0, False)
    only8 = [0] + [8] * 256
    add("dynamic HCLEN 5", dynamic(only8, [0], [1, 255, "E"], hclen=5, cl_lens=lens_of(19, s8=1, s0=2, s18=3, s16=4, s17=4), seq=[(0, 0)] + [(8, 0)] * 256 + [(0, 0)]), 2, True)
    add("dynamic HLIT 257, no distance code, literals only", dynamic(lens_of(257, s97=1, s98=2, s256=2), [0], [A, B, A, "E"]), 3, True)
    add("dynamic no distance code, a length used", dynamic(LIT3, [0], [A, 257, ("b", 0, 1), "E"]), 4, False)
    lit286 = lens_of(286, s97=1, s256=2, s285=2)
    add("dynamic HLIT 286", dynamic(lit286, [1, 1], [A, ("m", 258, 1), "E"]), 259, True)
    for f in (30, 31):
        add("dynamic HLIT field %d" % f, dynamic(lit286, [1, 1], [A, "E"], hlit=f), 1, False)
    add("dynamic HDIST 1, one distance code of length 1", dynamic(LIT3, [1], [A, ("m", 3, 1), "E"]), 4, True)
    add("dynamic one distance code, its unassigned sibling used", dynamic(LIT3, [1], [A, 257, ("b", 1, 1), "E"]), 4, False)
    dist30 = [1] + [0] * 28 + [1]
    add("dynamic HDIST 30", dynamic(LIT3, dist30, [A, ("m", 3, 1), "E"]), 4, True)
    for f in (30, 31):
        add("dynamic HDIST field %d" % f, dynamic(LIT3, dist30, [A, "E"], hdist=f), 1, False)
    for sym, lit, dist, ops in ((16, lens_of(260, s97=1, s256=2, s258=3, s259=3), [3, 3, 2, 1], [A, A, ("m", 4, 1), "E"]),
                                (17, LIT3 + [0, 0], [0, 0, 1, 1], [A, A, A, A, ("m", 3, 3), "E"]), (18, LIT3 + [0] * 8, [0, 0, 0, 1, 1], [A, A, A, A, A, ("m", 3, 4), "E"])):
        assert any(s == sym and i < len(lit) < i + k for s, e, i, k in rle(lit + dist)), sym
        add("dynamic repeat %d crossing into the distance lengths" % sym, dynamic(lit, dist, ops), sum(1 if isinstance(o, int) else o[1] for o in ops[:-1]), True)
    add("dynamic repeat 16 first", dynamic(LIT3, [1, 1], [A, "E"], seq=[(16, 0)] + rle(LIT3 + [1, 1])), 1, False)
    add("dynamic repeat past the end", dynamic(LIT3, [1, 1], [A, "E"], seq=rle(LIT3 + [1]) + [(1, 0), (16, 0)]), 1, False)
    add("dynamic zero repeat past the end", dynamic(LIT3, [1, 1], [A, "E"], seq=rle(LIT3 + [1, 1])[:-2] + [(18, 0)]), 1, False)
    add("dynamic no end-of-block code", dynamic(lens_of(257, s97=1, s98=1), [0], [A, B]), 2, False)
    add("dynamic over-subscribed literal/length set", dynamic(lens_of(257, s97=1, s98=1, s256=1), [0], [A, "E"]), 1, False)
    add("dynamic over-subscribed distance set", dynamic(LIT3, [1, 1, 1], [A, "E"]), 1, False)
    add("dynamic over-subscribed code-length set", dynamic(LIT3, [1, 1], [A, "E"], cl_lens=[4] * 14 + [5] * 5), 1, False)
    add("dynamic incomplete literal/length set", dynamic(lens_of(257, s97=2, s256=2), [0], [A, "E"]), 1, False)
    add("dynamic incomplete distance set", dynamic(LIT3, [2, 2], [A, "E"]), 1, False)
    add("dynamic incomplete code-length set", dynamic(LIT3, [1, 1], [A, "E"], cl_lens=[4] * 12 + [5] * 7), 1, False)
    add("dynamic one literal/length code of length 1", dynamic(lens_of(257, s256=1), [0], ["E"]), 0, True)
    add("dynamic one literal/length code, its unassigned sibling used", dynamic(lens_of(257, s256=1), [0], [("b", 1, 1), "E"]), 0, False)
    long_lit = lens_of(258, s97=15, s98=15, s256=1, s257=2, **{"s%d" % (99 + i): 3 + i for i in range(12)})
    long_dist = [15, 15, 1, 2] + [3 + i for i in range(12)]
    add("dynamic 15-bit literal and distance codes", dynamic(long_lit, long_dist, [A, B, 99, 110, ("m", 3, 1), ("m", 3, 2), ("m", 3, 3), "E"]), 13, True)
    # ---- the bit reader
    abc = fixed([A, B, 99, "E"]).done()
    add("input ends inside a symbol", abc[:3], 3, False)
    add("input ends inside the end-of-block code", abc[:4], 3, False)
    w = fixed([200, A, ("m", 131 + 31, 1), "E"])
    add("input ends inside extra bits", w.done()[:4], 2 + 162, False)
    add("input ends inside a dynamic header", dynamic(LIT3, [1, 1], [A, "E"]).done()[:5], 1, False)
    add("input ends inside the code lengths", dynamic(LIT3, [1, 1], [A, "E"]).done()[:14], 1, False)
    add("no input at all", b"", 0, False)
    w = fixed([200] * 6 + ["E"])
    assert w.n == 64
    add("the last symbol ends on the last bit of the last byte", w, 6, True)
    add("trailing garbage behind the final block", abc + b"\xff\x00\xff", 3, True)
    assert len({x[0] for x in c}) == len(c)
    return c


def text_like(n, rng):
    words = [b"chr1", b"ACGTTGCA", b"read", b"\t", b"IIIIIIII", b"100M", b"NM:i:0", b"\n", b"GATTACA", b"255"]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words)
    return bytes(out[:n])


def bam_blocks(path=FIXTURE_BAM):
    """[(deflate stream, ISIZE)] of every BGZF block of a file (header layout restated from the SAM specification, 4.1)"""
    raw, at, out = open(path, "rb").read(), 0, []
    while at < len(raw):
        xlen, = struct.unpack_from("<H", raw, at + 10)
        bsize, = struct.unpack_from("<H", raw, at + 16)
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 12:at + 14] == b"BC" and xlen == 6
        out.append((raw[at + 18:at + bsize + 1 - 8], struct.unpack_from("<I", raw, at + bsize + 1 - 4)[0]))
        at += bsize + 1
    return out


@functools.lru_cache(maxsize=None)
def zlib_cases():
    rng = random.Random(11)
    c = []
    for n in (1, 255, 256, 4097, 65536):
        for kind, data in (("random", rng.randbytes(n)), ("constant", b"\x41" * n), ("text", text_like(n, rng))):
            for level in (0, 1, 6, 9):
                for sname, strategy in (("default", zlib.Z_DEFAULT_STRATEGY), ("fixed", zlib.Z_FIXED), ("huffman", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)):
                    z = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
                    c.append(("zlib %d %s level %d %s" % (n, kind, level, sname), z.compress(data) + z.flush(), n))
    for i, (s, isize) in enumerate(bam_blocks()):
        c.append(("single-end.bam block %d" % i, s, isize))
    return c


@functools.lru_cache(maxsize=None)
def mutations(count=2000, seed=MUTATION_SEED):
    """flips in the valid streams of at most 8 KiB (the hand-built ones, zlib's and the fixture's blocks), so that the list stays a few megabytes"""
    rng = random.Random(seed)
    base = [(n, s, o) for n, s, o, ok in hand_cases() if ok and 0 < len(s) <= 8192] + [x for x in zlib_cases() if 0 < len(x[1]) <= 8192]
    out = []
    for k in range(count):
        name, s, o = base[rng.randrange(len(base))]
        b = bytearray(s)
        flips = [rng.randrange(8 * len(b)) for _ in range(rng.randint(1, 3))]
        for f in flips:
            b[f >> 3] ^= 1 << (f & 7)
        out.append(("mutation %d of %s: bits %s" % (k, name, flips), bytes(b), o))
    return out


def pack(cases, pad_src=0, pad_dst=0):
    """streams and destinations laid end to end -> (src bytes, descriptors as a structured numpy array, dst size).  pad_*: bytes left between neighbours"""
    dt = np.dtype([("src_offset", "<u8"), ("dst_offset", "<u8"), ("src_bytes", "<u4"), ("out_bytes", "<u4")])
    blocks = np.zeros(len(cases), dt)
    src, s_at, d_at = bytearray(), 0, 0
    for i, case in enumerate(cases):
        stream, out_bytes = case[1], case[2]
        blocks[i] = (s_at, d_at, len(stream), out_bytes)
        src += stream + b"\xa5" * pad_src
        s_at += len(stream) + pad_src
        d_at += out_bytes + pad_dst
    return bytes(src), blocks, d_at
