"""The record decoder of canvas_amd/csrc/bam_record.hpp on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/bam_record_host.cpp reads a chunk
into a heap buffer of exactly its size, decodes every offset and touches the ends of every part the decoder vouches for.  A byte read past the chunk ends the program —
the check the GPU tests cannot make, because a device allocation is rounded up.  The fields of good records are compared with hits_ref.decode_record; the damaged
records and stray offsets are the lists the GPU tests use (hits_ref.damaged_records, hits_ref.stray_offsets)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import hits_ref as H

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
M36 = [(36, "M")]


def rd(pos, ref=0, flag=0, cigar=M36, tlen=0, **kw):
    d = dict(ref=ref, pos=pos, flag=flag, cigar=cigar, seq="ACGT" * 9, tlen=tlen, mate_ref=ref, mate_pos=pos + 100)
    if cigar is not M36:
        d["seq"] = "A" * sum(k for k, o in cigar if o in "MIS=X")
    d.update(kw)
    return d


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("bam_record_host")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked statically where the compiler can: the program then runs whatever else the environment loads into a process
    for runtime in (["-static-libasan", "-static-libubsan"], []):
        p = subprocess.run([cxx] + SANITIZE + runtime + [str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
        if p.returncode == 0:
            break
    else:
        pytest.skip("%s cannot link the sanitizer runtimes: %s" % (cxx, p.stderr.strip()[-200:]))
    exe = tmp / "bam_record_host"
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + SANITIZE + runtime + [os.path.join(HERE, "bam_record_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return str(exe), tmp


def run(program, buf, offs, nbytes):
    """-> the program's lines for the chunk buf[:nbytes] (no byte behind it) and the offsets"""
    exe, tmp = program
    path = tmp / "chunk.bin"
    offs = np.asarray(offs, np.int64).astype(np.uint64)
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", nbytes, len(offs)) + offs.tobytes() + bytes(buf[:nbytes]))
    p = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert len(lines) == len(offs)
    return lines


def ends(raw, at, n):
    return [-1, -1] if n <= 0 else [raw[at], raw[at + n - 1]]


def expected(raw, at):
    """the line of the good record at `at`: the fields as hits_ref.decode_record reads them; the lengths, which it does not return, from the fixed bytes"""
    r, nxt = H.decode_record(raw, at)
    lname, ncig, lseq, nref, npos = struct.unpack_from("<B3xH2xiii", raw, at + 12)
    bs = nxt - at - 4
    assert len(r["cigar"]) == ncig and len(r["seq"]) == max(lseq, 0) and len(r["name"]) == max(lname - 1, 0)
    seq = lseq >= 0 and 32 + lname + 4 * ncig + (lseq + 1) // 2 + lseq <= bs
    out = [bs, r["ref"], r["pos"], lname, r["mapq"], ncig, r["flag"], lseq, nref, npos, r["tlen"], int(seq)]
    p = at + 36
    out += ends(raw, p, lname) + ends(raw, p + lname, 4 * ncig)
    p += lname + 4 * ncig
    out += ends(raw, p, (lseq + 1) // 2 if seq else 0) + ends(raw, p + (lseq + 1) // 2, lseq if seq else 0)
    return "ok " + " ".join(str(int(x)) for x in out)


def check(program, reads, bad=(), extra_offsets=(), nbytes=None):
    """reads through chunk_of with no padding; the offsets at the indices in `bad` must come out malformed, every other one as decode_record reads it"""
    buf, offs, used = H.chunk_of(reads, 0, extra_offsets)
    nbytes = used if nbytes is None else nbytes
    raw = bytes(buf[:nbytes])
    lines = run(program, buf, offs, nbytes)
    for i, (line, off) in enumerate(zip(lines, offs)):
        assert line == ("malformed" if i in bad else expected(raw, int(off))), (i, int(off), line)
    return lines


GOOD = [rd(3, tlen=10, name="first"), rd(4, tlen=-20, flag=0x63, mapq=7), rd(4, tlen=30, cigar=[(5, "S"), (31, "M"), (2, "D")], qual=list(range(36)))]


def test_good_records(program):
    lines = check(program, GOOD)
    assert all(ln.startswith("ok ") and ln.split()[12] == "1" for ln in lines)
    check(program, [])


def test_edges_of_the_fields(program):
    """every case is the LAST record of a chunk with nothing behind it (and the first of another one)"""
    cases = {
        "l_read_name 0": rd(9, name="", l_read_name=0),                       # (the NUL the encoder writes is then the CIGAR's first byte)
        "l_read_name 1": rd(9, name=""),
        "l_read_name 255": rd(9, name="n" * 254),
        "n_cigar_op 0": rd(9, cigar=[], seq="ACG"),
        "n_cigar_op 65535": rd(9, cigar=[(1, "M")] * 65535, seq=""),
        "l_seq 0": rd(9, seq="", cigar=[(3, "D")]),
        "odd l_seq": rd(9, seq="ACGTA", cigar=[(5, "M")]),
        "negative l_seq": rd(9, seq="", l_seq=-1),
        "l_seq past block_size": rd(9, seq="ACGT", l_seq=5),
        "extreme values": rd(-(2 ** 31), ref=-1, flag=0xFFFF, mapq=255, tlen=-(2 ** 31), mate_ref=2 ** 31 - 1, mate_pos=-1),
    }
    for what, r in cases.items():
        lines = check(program, GOOD + [r]) + check(program, [r] + GOOD)
        holds = what not in ("negative l_seq", "l_seq past block_size")
        assert lines[3].split()[12] == lines[4].split()[12] == ("1" if holds else "0"), what
    # block_size 32 and nothing else: the 36 bytes a record needs at the least are the whole chunk (the encoder's NUL is cut off)
    least = rd(9, name="", l_read_name=0, cigar=[], seq="", block_size=32)
    lines = check(program, [least], nbytes=36)
    assert lines[0].split()[1] == "32" and lines[0].split()[13:] == ["-1"] * 8
    check(program, GOOD + [least], nbytes=sum(len(H.encode_record(r)) for r in GOOD) + 36)
    check(program, [least], bad=[0], nbytes=35)
    # a block_size that ends exactly at nbytes, and one byte behind it
    last = rd(9)
    size = sum(len(H.encode_record(r)) for r in GOOD + [last])
    check(program, GOOD + [last], nbytes=size)
    check(program, GOOD + [last], bad=[3], nbytes=size - 1)


def test_damaged_records(program):
    for what, bad, last_only in H.damaged_records(rd):
        check(program, GOOD + [bad], bad=[3])
        if not last_only:
            check(program, [bad] + GOOD, bad=[0])


def test_stray_offsets(program):
    nbytes = sum(len(H.encode_record(r)) for r in GOOD)
    for what, off in H.stray_offsets(nbytes):
        for idx in (0, 2, 3):
            check(program, GOOD, bad=[idx], extra_offsets=[(idx, off)])
    # an offset inside a record that leaves 36 bytes: whatever stands there is decoded, and nothing outside the chunk is read
    buf, offs, used = H.chunk_of(GOOD)
    run(program, buf, list(range(0, used - 35)), used)
