"""The deflate decoder and the BGZF block walk of canvas_amd/csrc/inflate_block.hpp on the host, under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/inflate_host.cpp puts every stream of tests/deflate_cases.py into a heap buffer of exactly its size and inflates it into one of exactly out_bytes, so a byte read
or written outside either ends the program — the check the GPU test cannot make, because a device allocation is rounded up.  Status 0 exactly where zlib accepts, and
zlib's bytes there.  The block walk is compared with a restatement of bgzf_parse (canvas_amd/tools/bam_io.hpp) in Python."""
import os
import shutil
import struct
import subprocess
import zlib

import pytest

import deflate_cases as D

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("inflate_host")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked statically where the compiler can: the program then runs whatever else the environment loads into a process
    for runtime in (["-static-libasan", "-static-libubsan"], []):
        p = subprocess.run([cxx] + SANITIZE + runtime + [str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
        if p.returncode == 0:
            break
    else:
        pytest.skip("%s cannot link the sanitizer runtimes: %s" % (cxx, p.stderr.strip()[-200:]))
    exe = tmp / "inflate_host"
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + SANITIZE + runtime + [os.path.join(HERE, "inflate_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return str(exe), tmp


def inflate(program, cases):
    """-> [(status, bytes)] of (name, stream, out_bytes, ...) cases"""
    exe, tmp = program
    with open(tmp / "cases.bin", "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for case in cases:
            f.write(struct.pack("<II", len(case[1]), case[2]) + case[1])
    p = subprocess.run([exe, "inflate", str(tmp / "cases.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-3000:])
    raw, at, out = open(tmp / "out.bin", "rb").read(), 0, []
    for case in cases:
        st, = struct.unpack_from("<i", raw, at)
        at += 4
        n = case[2] if st == 0 else 0
        out.append((st, raw[at:at + n]))
        at += n
    assert at == len(raw)
    return out


def check(program, cases):
    got = inflate(program, cases)
    for case, (st, data) in zip(cases, got):
        ok, want, refused = D.expected_status(case[1], case[2])
        assert (st == 0) == ok and (st == 1) == refused, (case[0], st)
        if ok:
            assert data == want, case[0]
    return got


def test_hand_built_cases(program):
    cases = D.hand_cases()
    got = check(program, cases)
    for (name, s, o, accepted), (st, data) in zip(cases, got):
        assert (st == 0) == (accepted and len(s) <= D.LIMIT), name      # ("stored 65535" is valid deflate and longer than a BGZF block may be)
    # the status names the rule where one stream breaks one rule only
    by = {c[0]: st for c, (st, data) in zip(cases, got)}
    for name, st in (("BTYPE 3", 2), ("stored LEN != ~NLEN", 2), ("dynamic HLIT field 30", 2), ("dynamic HDIST field 31", 2), ("stored length beyond the input", 3),
                     ("input ends inside a symbol", 3), ("no input at all", 3), ("overrun by one byte from a match", 4), ("overrun by one byte from a literal", 4),
                     ("stored length beyond out_bytes", 4), ("one byte short of out_bytes", 5), ("distance one more than the bytes produced", 6),
                     ("fixed literal/length symbol 286", 7), ("fixed distance symbol 31", 7), ("dynamic repeat 16 first", 7), ("dynamic no end-of-block code", 7),
                     ("dynamic over-subscribed distance set", 7), ("dynamic incomplete literal/length set", 7), ("dynamic one distance code, its unassigned sibling used", 7)):
        assert by[name] == st, (name, by[name])


def test_zlib_output_and_the_fixture_bam(program):
    got = check(program, D.zlib_cases())
    assert sum(st == 0 for st, data in got) > 200 and any(st == 1 for st, data in got)


def test_mutations(program):
    muts = D.mutations()
    accepted = sum(D.zlib_verdict(s, o)[0] for n, s, o in muts)
    assert accepted >= 100 and len(muts) - accepted >= 100
    check(program, muts)


def test_sizes_beyond_the_bound(program):
    got = inflate(program, [("src 65537", D.stored(b"").done() + bytes(65532), 0), ("out 65537", b"\x03\x00", 65537)])
    assert [st for st, data in got] == [1, 1]


# ---- the block walk
def bgzf_block(data, level=6, extra_before=b"", extra_after=b"", isize=None, bsize=None):
    z = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = z.compress(data) + z.flush()
    extra = extra_before + b"BC\x02\x00\x00\x00" + extra_after
    size = 12 + len(extra) + len(body) + 8
    extra = bytearray(extra)
    extra[len(extra_before) + 4:len(extra_before) + 6] = struct.pack("<H", size - 1 if bsize is None else bsize)
    return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", len(extra)) + bytes(extra) + body + struct.pack("<II", zlib.crc32(data), len(data) if isize is None else isize)


def parse(h):
    """bgzf_parse restated -> (size, data offset, data bytes, isize), or None for bytes that are no whole block"""
    if len(h) < 12 or h[0] != 31 or h[1] != 139 or h[2] != 8 or not h[3] & 4:
        return None
    xlen, = struct.unpack_from("<H", h, 10)
    if len(h) < 12 + xlen:
        return None
    bsize, i = -1, 0
    while i + 4 <= xlen:
        slen, = struct.unpack_from("<H", h, 12 + i + 2)
        if h[12 + i:12 + i + 2] == b"BC" and slen == 2 and i + 6 <= xlen:
            bsize, = struct.unpack_from("<H", h, 12 + i + 4)
        i += 4 + slen
    if bsize < 0 or bsize + 1 < 12 + xlen + 8 or len(h) < bsize + 1:
        return None
    isize, = struct.unpack_from("<I", h, bsize + 1 - 4)
    return (bsize + 1, 12 + xlen, bsize + 1 - 12 - xlen - 8, isize) if isize <= 65536 else None


def scan_ref(raw, at, max_out, capacity):
    blocks, total = [], 0
    while True:
        if len(blocks) >= capacity or total >= max_out:
            why = 0
            break
        if at >= len(raw):
            why = 1
            break
        p = parse(raw[at:])
        if p is None:
            why = 2
            break
        blocks.append((at + p[1], total, p[2], p[3]))
        total += p[3]
        at += p[0]
    return [len(blocks), at, total, why], blocks


def scan(program, raw, at=0, max_out=(1 << 64) - 1, capacity=1000):
    exe, tmp = program
    with open(tmp / "file.bin", "wb") as f:
        f.write(raw)
    p = subprocess.run([exe, "scan", str(tmp / "file.bin"), str(at), str(max_out), str(capacity)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-3000:])
    lines = [[int(x) for x in ln.split()] for ln in p.stdout.splitlines()]
    got = (lines[0], [tuple(b) for b in lines[1:]])
    assert got == scan_ref(raw, at, max_out, capacity)
    return got


def test_block_walk(program):
    a, b, c = bgzf_block(b"first block " * 50), bgzf_block(b"", level=0), bgzf_block(b"third" * 1000, level=1)
    eof = bgzf_block(b"")
    info, blocks = scan(program, a + b + c + eof)
    assert info == [4, len(a + b + c + eof), 600 + 5000, 1] and [x[3] for x in blocks] == [600, 0, 5000, 0]
    assert zlib.decompressobj(-15).decompress((a + b + c)[blocks[2][0]:blocks[2][0] + blocks[2][2]]) == b"third" * 1000
    assert scan(program, a + b + c, at=len(a))[0] == [2, len(a + b + c), 5000, 1]
    assert scan(program, b"")[0] == [0, 0, 0, 1]
    # subfields before and behind BC; XLEN 0; a BC of another length
    assert scan(program, bgzf_block(b"x" * 9, extra_before=b"AB\x03\x00abc") + bgzf_block(b"y", extra_after=b"ZZ\x00\x00") + a)[0][0] == 3
    assert scan(program, a + b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x00\x00" + bytes(40))[0] == [1, len(a), 600, 2]
    assert scan(program, a + b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x07\x00BC\x03\x00\x30\x00\x00" + bytes(40))[0] == [1, len(a), 600, 2]
    assert scan(program, a + b"\x1f\x8b\x08\x00" + bytes(40))[0][3] == 2             # no FEXTRA
    assert scan(program, a + b"\x1f\x8b\x07\x04" + bytes(40))[0][3] == 2
    # BSIZE too small for header and trailer; ISIZE 65537 and 65536
    assert scan(program, a + bgzf_block(b"q", bsize=24) + c)[0] == [1, len(a), 600, 2]
    assert scan(program, bgzf_block(b"q", isize=65537) + c)[0] == [0, 0, 0, 2]
    assert scan(program, bgzf_block(b"q", isize=65536) + c)[0][0] == 2
    # the file ends inside a header, inside the extra field, inside a block, one byte short
    for cut in (5, 11, 12, 15, 17, 18, 30, len(c) - 1):
        assert scan(program, a + c[:cut])[0] == [1, len(a), 600, 2], cut
    # stops: capacity, max_out_bytes (reached, not exceeded by design: the block that reaches it is the last)
    assert scan(program, a + b + c, capacity=2)[0] == [2, len(a + b), 600, 0]
    assert scan(program, a + b + c, capacity=0)[0] == [0, 0, 0, 0]
    assert scan(program, a + b + c, max_out=600)[0] == [1, len(a), 600, 0]
    assert scan(program, a + b + c, max_out=601)[0] == [3, len(a + b + c), 5600, 0]
    assert scan(program, a + b + c, max_out=0)[0] == [0, 0, 0, 0]
    assert scan(program, open(D.FIXTURE_BAM, "rb").read())[0][3] == 1
